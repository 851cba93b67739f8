"""The reset layer on the GPU as raw bytes: for a refactor of build_reset_pool / AssistiveVecEnv's pool handling / the scalar reset() bodies that
must not change a state.  Per model of MODELS:
  * pool/device, pool/host: build_reset_pool(blob, n, seed=1001, sampler=...) -- n = 8, or 2 for the models with a garment or water (their array
    is hashed as `.../cloth`);
  * device/reset, device/boundary: the state tensor after AssistiveVecEnv(n, reset='device').reset(), and after EPISODE_LEN + 1 zero-action steps
    (one in-place masked agx_reset at the episode boundary) -- on a copy of the blob whose EPISODE_LEN task word is 4.
Writes {case: sha256} as JSON and the arrays themselves next to it (.npz: a case that does not reproduce on one tree is compared at a tolerance).
Uses only names both trees have; run it in a fresh process per tree.
usage: python tools/gpu_reset_bits.py out.json [MODEL ...];   python tools/gpu_reset_bits.py --compare a.json b.json"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = ('feeding_jaco', 'feeding_sawyer', 'drinking_jaco', 'scratch_itch_jaco', 'scratch_itch_pr2', 'bed_bathing_sawyer', 'arm_manipulation_sawyer', 'dressing_baxter')
SEED, SHORT_EPISODE = 1001, 4


def short_episode(blob):
    """a copy of the blob whose episodes last SHORT_EPISODE steps (the EPISODE_LEN word of the task section)"""
    from assistive_gym_amd.blob import ModelBlob
    from assistive_gym_amd.model import compiler as L
    w = blob.words.copy()
    w.view(np.float32)[blob.h['OFF_TASK'] + L.T['EPISODE_LEN']] = SHORT_EPISODE
    return ModelBlob(w, blob.meta)


def cases(model):
    import torch
    from assistive_gym_amd.blob import ModelBlob
    from assistive_gym_amd.vec_env import AssistiveVecEnv, build_reset_pool
    blob = ModelBlob.load(model)
    n = 2 if model.startswith(('dressing', 'drinking')) else 8
    out = {}
    for sampler in ('device', 'host'):
        if sampler == 'device' and not blob.has_reset_generator:
            continue
        pool = build_reset_pool(blob, n, seed=SEED, sampler=sampler)
        states, cloth = pool if isinstance(pool, tuple) else (pool, None)
        out['%s/pool/%s/states' % (model, sampler)] = states
        if cloth is not None:
            out['%s/pool/%s/cloth' % (model, sampler)] = cloth
    if blob.has_reset_generator:
        env = AssistiveVecEnv(n, blob=short_episode(blob), seed=SEED, reset='device')
        env.reset()
        torch.cuda.synchronize()
        out[model + '/device/reset/states'] = env.stepper.get_state()
        zero = torch.zeros((n, env.act_dim), dtype=torch.float32, device=env.device)
        for _ in range(SHORT_EPISODE + 1):
            env.step(zero)
        torch.cuda.synchronize()
        out[model + '/device/boundary/states'] = env.stepper.get_state()
        out[model + '/device/boundary/episodes'] = np.array([env._episode], dtype=np.int32)
        if env.stepper.cloth_nodes() > 0:
            out[model + '/device/boundary/cloth'] = env.stepper.get_cloth()
        env.close()
    return out


def main():
    if sys.argv[1] == '--compare':
        a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        for k in bad:
            print('differs:', k)
        print('%d cases: %s' % (len(a), 'IDENTICAL' if not bad else 'DIFFERENT (%d cases)' % len(bad)))
        sys.exit(1 if bad else 0)
    arrays = {}
    for model in sys.argv[2:] or MODELS:
        arrays.update(cases(model))
        print('done:', model, flush=True)
    json.dump({k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in arrays.items()}, open(sys.argv[1], 'w'), indent=1, sort_keys=True)
    np.savez_compressed(os.path.splitext(sys.argv[1])[0] + '.npz', **arrays)
    print('wrote %s: %d cases' % (sys.argv[1], len(arrays)))


if __name__ == '__main__':
    main()
