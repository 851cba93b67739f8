"""Timing of end-effector control on the device (profiles/ee_control/README.md): agx_ee_ik alone at 4,096 FeedingJaco environments for iters = 1, 8 and
200 (device events around windows of back-to-back calls, after warm-up), and 200 env steps through ee_control.EndEffectorControl against 200 plain
steps of the same env in the same process, alternating (host clock around work that ends in a device synchronise).

    python tools/gpu_ee_timing.py [--envs 4096] [--out FILE.json]

Two kinds of command are timed for every iteration count: 'delta' -- random end-effector deltas of up to 1 cm / 0.05 rad, what a policy sends: most
environments stop before the iteration budget is spent and a wavefront leaves the loop when its last lane has -- and 'far' -- an absolute target 5 m
away that no environment reaches: every iteration runs."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_calls(fn, reps, windows=3):
    """ms per call of `reps` back-to-back calls between two device events, `windows` times"""
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from assistive_gym_amd.ee_control import EndEffectorControl
    from assistive_gym_amd.vec_env import FeedingJacoVecEnv
    n = args.envs
    inner = FeedingJacoVecEnv(n, seed=1001)
    env = EndEffectorControl(inner)
    env.reset()
    g = torch.Generator(device='cuda'); g.manual_seed(1)
    st, stream = inner.stepper, inner._stream()
    result = dict(n_envs=n, device=torch.cuda.get_device_name(0), ik_ms={}, steps=args.steps)
    delta = (torch.rand((n, 6), device='cuda', generator=g) * 2 - 1) * env._scale
    far = env.ee_pose().clone().reshape(n, 7)
    far[:, 0] += 5.0
    action = torch.zeros((n, inner.act_dim), device='cuda')
    err = torch.zeros((n, 1, 2), device='cuda')
    for iters in (1, 8, 200):
        for name, target, frame in (('delta', delta, 'delta'), ('far', far, 'absolute')):
            fn = lambda: st.ee_ik(target, frame, iters=iters, action=action, err=err, stream=stream)
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            ms = time_calls(fn, 400 if iters < 200 else 40)
            stopped = float((err[:, 0, :] < 1e-4).all(dim=1).float().mean())
            result['ik_ms']['%s_iters%d' % (name, iters)] = dict(ms_per_call=ms, share_below_tolerance_at_exit=stopped)
            print('agx_ee_ik %-5s iters=%-3d: %s ms per call (%.0f %% of the environments below the tolerance at exit)' % (name, iters, ', '.join('%.4f' % m for m in ms), 100 * stopped), flush=True)
    # what the wrapper puts in front of a step: the command's clamp / scale / copy (torch) and the IK launch
    one = torch.rand((n, env.act_dim), device='cuda', generator=g) * 2 - 1
    for _ in range(10):
        env.joint_action(one)
    result['joint_action_ms'] = time_calls(lambda: env.joint_action(one), 400)
    print('EndEffectorControl.joint_action (torch clamp / scale + agx_ee_ik, iters=%d): %s ms per call' % (env.iters, ', '.join('%.4f' % m for m in result['joint_action_ms'])), flush=True)
    # 200 plain steps against 200 steps through the wrapper, alternating, a fresh uniform action / command every step (bench.py's random-policy rollout)
    plain = torch.rand((args.steps, n, inner.act_dim), device='cuda', generator=g) * 2 - 1
    cmd = torch.rand((args.steps, n, env.act_dim), device='cuda', generator=g) * 2 - 1
    for k in range(20):
        inner.step(plain[k]); env.step(cmd[k])
    rounds = dict(plain=[], wrapped=[])
    for _ in range(3):
        for name, fn, a in (('plain', inner.step, plain), ('wrapped', env.step, cmd)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                fn(a[k])
            torch.cuda.synchronize()
            rounds[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    result['ms_per_step'] = rounds
    print('ms per step over %d steps, three alternating rounds: plain %s, through the wrapper %s' % (args.steps, ', '.join('%.4f' % m for m in rounds['plain']), ', '.join('%.4f' % m for m in rounds['wrapped'])), flush=True)
    env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
