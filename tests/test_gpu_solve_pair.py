"""-m gpu: two environments per wavefront in the solve kernel (csrc/agx_pgs_lvw.h pgs_lvw_pair, AGX_SOLVE_PAIR -- the default of the feeding variant) against
lib/variants/solo.so, the same library with one environment per wavefront (-DAGX_SOLVE_PAIR=0, built by __graft_entry__.build()).  Each environment of a pair
visits its rows in the order it would alone, so states, observations, rewards and info come out IDENTICAL, bit for bit: with chunk sizes that leave an
environment without a partner, with other pairings (AGX_CHUNKS), with far rows in both halves (the smallest LDS window), with two friction directions, with
both halves on the narrow sweep (SOLVE_WIDE = 0), for FeedingPanda, for partners with very different row counts and through a masked agx_reset that splits
most pairs.  Each build runs in its own process (AGX_LIB)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = os.path.join(ROOT, 'tools', 'gpu_lv_bits.py')
PAIR = os.path.join(ROOT, 'tools', 'gpu_pair_bits.py')
SOLO = os.path.join(ROOT, 'assistive_gym_amd', 'lib', 'variants', 'solo.so')


def _run(args, env):
    e = dict(os.environ); e.update(env)
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    return r.stdout


def _identical(tmp_path, args_of, env):
    """the run of the default library and of solo.so under the same switches: every array bit-identical"""
    assert os.path.exists(SOLO), 'lib/variants/solo.so is missing: run __graft_entry__.build()'
    a, b = str(tmp_path / 'paired.npz'), str(tmp_path / 'solo.npz')
    out = _run(args_of(a), env)
    _run(args_of(b), dict(env, AGX_LIB=SOLO))
    r = subprocess.run([sys.executable, BITS, '--compare', a, b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'IDENTICAL' in r.stdout, r.stdout[-1500:]
    return out


# 129 environments: three chunks of 43 (the last environment of every chunk is alone), one of 129, two of 65 and 64 (other pairs: a partner does not leak)
@pytest.mark.parametrize('env', [{}, {'AGX_CHUNKS': '1'}, {'AGX_CHUNKS': '2'}, {'AGX_SOLVE_LDS_BYTES': '9536'}, {'AGX_BITS_PARAM': 'FRICTION_DIRS=2'},
                                 {'AGX_BITS_PARAM': 'SOLVE_WIDE=0'}], ids=lambda e: ','.join('%s=%s' % kv for kv in e.items()) or 'default')
def test_feeding_jaco_129_environments(tmp_path, env):
    _identical(tmp_path, lambda out: [BITS, out, '129', '40'], env)


def test_feeding_panda(tmp_path):
    _identical(tmp_path, lambda out: [BITS, out, '64', '20'], {'AGX_BITS_ENV': 'FeedingPandaVecEnv'})


def test_unequal_partners(tmp_path):
    """a scene with the food on the spoon beside one whose food falls freely, alternating: 16 environments x 20 steps"""
    out = _identical(tmp_path, lambda out: [PAIR, 'unequal', out, '16', '20'], {})
    assert 'rows per environment' in out


def test_masked_reset_splits_the_pairs(tmp_path):
    """agx_reset on every third environment, then 5 steps: the environments outside the mask keep their bits (checked by the tool), the batch equals solo.so"""
    _identical(tmp_path, lambda out: [PAIR, 'masked', out, '48', '5'], {})
