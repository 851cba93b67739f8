"""bench.py's host-side pieces that do not need a GPU: the usable-core detection and the CPU-oracle
worker processes of the `cpu_baseline` leg (kind = "port": the C restatement, never the product path)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_usable_cores():
    import bench
    n = bench._usable_cores()
    assert 1 <= n <= (os.cpu_count() or 1)


def test_cpu_baseline_leg(blob):
    import bench
    from assistive_gym_amd.host.reset import make_states
    st, _ = make_states(blob, 4, seed=11)
    r = bench.cpu_baseline(blob, st, 1, 3)
    assert r['kind'] == 'port' and r['unit'] == 'env-steps/s' and r['cores'] == bench._usable_cores()
    assert r['value'] > 0 and 'not PyBullet' in r['sample']


def test_wiping_pool_puts_the_pad_on_the_arm():
    """bench.py --task bedbathing --workload wiping (BASELINE config 3, 'dense tool-skin contact'): in every pool state the wiping pad
    touches the person's arm (a tool <-> human contact in the oracle's collision pass)"""
    import bench
    from assistive_gym_amd.blob import ModelBlob
    from oracle_lib import Oracle
    b = ModelBlob.load('bed_bathing_sawyer')
    st = bench.wiping_pool(b, 6, 1001)
    o = Oracle(b)
    hits = 0
    for s in st:
        con = o.collide(s)
        tags = [(b.collider(int(c[0]))['tag'], b.collider(int(c[1]))['tag']) for c in con]
        hits += any(set(t) == {2, 3} for t in tags)            # AGX_TAG_TOOL, AGX_TAG_HUMAN
    assert hits == len(st), (hits, len(st))


def test_dump_outputs_float32_and_bounded(tmp_path, monkeypatch):
    """--dump-outputs: every array as float32 (float64 kept); above the size limit every array keeps the same seeded share of its rows,
    with the picked rows beside it"""
    import bench
    a = {'obs': np.arange(40, dtype=np.float32).reshape(20, 2), 'done': np.ones(20, dtype=np.uint8), 'sum': np.zeros(10)}
    bench.dump_outputs(str(tmp_path / 'all'), a)
    got = {k: np.load(str(tmp_path / 'all' / (k + '.npy'))) for k in a}
    assert got['obs'].dtype == np.float32 and got['done'].dtype == np.float32 and got['sum'].dtype == np.float64
    assert np.array_equal(got['obs'], a['obs']) and np.array_equal(got['done'], a['done']) and not (tmp_path / 'all' / 'obs_rows.npy').exists()
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 200)
    for k in ('s0', 's1'):
        bench.dump_outputs(str(tmp_path / k), a)
    files = sorted(os.listdir(str(tmp_path / 's0')))
    assert files == ['done.npy', 'done_rows.npy', 'obs.npy', 'obs_rows.npy', 'sum.npy', 'sum_rows.npy']
    assert sum(os.path.getsize(str(tmp_path / 's0' / f)) - 128 for f in files) <= 200          # (128: the .npy header)
    rows = np.load(str(tmp_path / 's0' / 'obs_rows.npy')).astype(int)
    assert np.array_equal(np.load(str(tmp_path / 's0' / 'obs.npy')), a['obs'][rows])
    for f in files:
        assert np.array_equal(np.load(str(tmp_path / 's0' / f)), np.load(str(tmp_path / 's1' / f)))


def test_plain_dry_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    """a plain run (no --full) prints the headline fields alone; --dump-outputs writes what the last timed step returned; --steps is the
    number of timed steps (the launch path of bench.py on CPU tensors: --dry-run, one rank)"""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--dry-run', '--steps', '5', '--warmup', '2', '--envs-per-gpu', '16',
                        '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j['metric'] == 'env_steps_per_sec' and j['unit'] == 'env-steps/s' and j['higher_is_better'] is True and j['dtype'] == 'f32'
    assert j['steps'] == 5 and j['warmup'] == 2 and j['ms_per_step'] > 0 and j['value'] > 0
    assert not {'configs', 'cpu_baseline', 'roofline'} & set(j)
    out = {k: np.load(str(tmp_path / (k + '.npy'))) for k in ('obs', 'reward', 'done', 'info')}
    assert all(v.dtype == np.float32 for v in out.values())
    assert out['obs'].shape == (16, 25) and out['reward'].shape == (16,) and out['done'].shape == (16,) and out['info'].shape == (16, 8)
    assert np.array_equal(out['obs'][:, -1], np.arange(16)) and np.array_equal(out['reward'], -np.arange(16))
    # the stand-in echoes the step's actions into the observation: the dump holds the LAST timed step's (tape of bench.dry_run)
    import torch
    g = torch.Generator(); g.manual_seed(1001)
    tape = (torch.rand((2 + 5, 16, 7), generator=g) * 2 - 1).numpy()
    assert np.array_equal(out['obs'][:, :7], tape[-1]) and not np.array_equal(out['obs'][:, :7], tape[-2])
