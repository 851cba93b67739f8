"""The host reset layer (assistive_gym_amd/host/reset*.py) as raw bytes: for a refactor of the numpy samplers that must not move a draw.
For every model of MODELS it calls the task's make_states WITHOUT settler or checker (nothing here needs a device) and hashes
  * the state records, the garment / water array where the task has one, and the repr of the sorted info dictionaries,
  * for seed 77 and seed 1001 three states each with the task's default impairment, and one state (seed 77) per explicit impairment
    'none', 'limits', 'weakness', 'tremor' ('tremor' not for arm manipulation, whose human never trembles: arm_manipulation.py:112),
  * for the models of REDRAW the placement re-draw of init_robot_pose's rejection loop: sample(..., attempt=1) over the record of attempt 0
    (feeding, scratch itch, dressing), post_settle(..., attempt=1) for bed bathing -- the placement stream must not shift.
Only public names are used, so that the same file runs in two trees.  Run it in both and compare:
usage: python tests/diag/reset_layer_bits.py out.json [processes];  python tests/diag/reset_layer_bits.py --compare a.json b.json
       python tests/diag/reset_layer_bits.py --write-golden   (tests/golden/host_reset_records.npz: seed 77, two states per model; read by
       tests/test_host_reset_bits.py -- written from the tree whose records are the reference)"""
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

MODELS = ('feeding_jaco', 'feeding_sawyer', 'feeding_stretch', 'drinking_jaco', 'scratch_itch_pr2', 'scratch_itch_jaco', 'scratch_itch_stretch',
          'bed_bathing_sawyer', 'bed_bathing_jaco', 'dressing_baxter', 'dressing_stretch', 'arm_manipulation_sawyer', 'arm_manipulation_pr2')
REDRAW = ('feeding_sawyer', 'feeding_stretch', 'scratch_itch_pr2', 'scratch_itch_stretch', 'dressing_baxter', 'dressing_stretch', 'bed_bathing_sawyer')
SEEDS, N_STATES, IMPAIRMENT_SEED = (77, 1001), 3, 77
GOLDEN = os.path.join(TESTS, 'golden', 'host_reset_records.npz')
GOLDEN_SEED, GOLDEN_STATES = 77, 2


def sampler_module(model):
    import importlib
    task = model.rsplit('_', 1)[0]
    return importlib.import_module('assistive_gym_amd.host.' + {'feeding': 'reset', 'drinking': 'reset_drinking', 'scratch_itch': 'reset_scratch', 'bed_bathing': 'reset_bed',
                                                                'dressing': 'reset_dressing', 'arm_manipulation': 'reset_arm'}[task])


def sample(model, n, seed, impairment=None):
    """-> (state records, garment / water array or None, infos) of the task's make_states, no settler, no checker"""
    from assistive_gym_amd.blob import ModelBlob
    kw = {} if impairment is None else dict(impairment=impairment)
    out = sampler_module(model).make_states(ModelBlob.load(model), n, seed=seed, **kw)
    return (out[0], out[1], out[2]) if len(out) == 3 else (out[0], None, out[1])


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hashes(states, extra, infos):
    np.set_printoptions(precision=17, threshold=1 << 20, linewidth=200)
    r = {'states': _sha(states), 'info': hashlib.sha256(repr([sorted(i.items()) for i in infos]).encode()).hexdigest()}
    if extra is not None:
        r['extra'] = _sha(extra)
    return r


def redraw(model, seed=77):
    """attempt 0, then the placement re-draw (attempt 1) over the same record, as reject_collisions drives the samplers"""
    from assistive_gym_amd.blob import ModelBlob
    blob, mod = ModelBlob.load(model), sampler_module(model)
    row, info = blob.new_state(1), {}
    if model.startswith('bed_bathing'):
        rs, rng = mod.BedBathingSawyerReset(blob), np.random.RandomState(seed)
        pre = rs.pre_settle(rng)
        rs.post_settle(rng, row, pre, env_seed=seed, info=info)
        rs.post_settle(rng, row, pre, env_seed=seed, info=info, attempt=1)
        return _hashes(row, None, [info])
    extra = None
    if model.startswith('dressing'):
        rs, extra = mod.DressingReset(blob), np.zeros((2, mod.cloth_nodes(blob), 3), dtype=np.float32)
    else:
        rs = mod.ScratchItchReset(blob) if model.startswith('scratch') else mod.FeedingJacoReset(blob)
    for attempt in (0, 1):
        args = (np.random.RandomState(seed), row) + (() if extra is None else (extra,))
        rs.sample(*args, env_seed=seed, info=info, attempt=attempt)
    return _hashes(row, extra, [info])


def run(model):
    t0, out = time.time(), {}
    for seed in SEEDS:
        out['%s/seed%d' % (model, seed)] = _hashes(*sample(model, N_STATES, seed))
    for imp in ('none', 'limits', 'weakness', 'tremor'):
        if imp == 'tremor' and model.startswith('arm_manipulation'):
            continue
        out['%s/%s' % (model, imp)] = _hashes(*sample(model, 1, IMPAIRMENT_SEED, imp))
    if model in REDRAW:
        out['%s/attempt1' % model] = redraw(model)
    return out, model, time.time() - t0


def write_golden():
    res = {}
    for m in MODELS:
        st, extra, _ = sample(m, GOLDEN_STATES, GOLDEN_SEED)
        res[m + '/states'] = st.view(np.uint32)                  # raw words: a float32 NaN pattern would survive too
        if extra is not None:
            res[m + '/extra_sha256'] = np.frombuffer(bytes.fromhex(_sha(extra)), dtype=np.uint8)
    np.savez_compressed(GOLDEN, **res)
    print('wrote %s: %d models, %d bytes' % (GOLDEN, len(MODELS), os.path.getsize(GOLDEN)))


def main():
    if sys.argv[1] == '--compare':
        a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        for k in bad:
            print('differs:', k)
        print('%d cases: %s' % (len(a), 'IDENTICAL' if not bad else 'DIFFERENT (%d cases)' % len(bad)))
        sys.exit(1 if bad else 0)
    if sys.argv[1] == '--write-golden':
        return write_golden()
    from multiprocessing import Pool
    res = {}
    with Pool(int(sys.argv[2]) if len(sys.argv) > 2 else 8) as pool:
        for r, model, dt in pool.imap_unordered(run, MODELS):
            res.update(r)
            print('%-26s %6.1f s' % (model, dt), flush=True)
    json.dump(res, open(sys.argv[1], 'w'), indent=1, sort_keys=True)
    print('wrote %s: %d cases' % (sys.argv[1], len(res)))


if __name__ == '__main__':
    main()
