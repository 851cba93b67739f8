"""GPU box: FeedingJaco runs that put UNEQUAL or MISSING partners into the workgroups of the paired solve kernel (csrc/agx_pgs_lvw.h pgs_lvw_pair), for a
bit-for-bit comparison of the default library with lib/variants/solo.so (one environment per wavefront); compare with tools/gpu_lv_bits.py --compare.
usage: AGX_LIB=<build> python tools/gpu_pair_bits.py unequal out.npz [n_envs] [steps]
           environments alternate between a settled scene with the food on the spoon and the same kind of scene whose food has been moved a metre aside and
           falls freely (far fewer rows): every workgroup pairs a long list of steps with a short one;
       AGX_LIB=<build> python tools/gpu_pair_bits.py masked out.npz [n_envs] [steps]
           agx_reset on a mask that selects every third environment (most pairs are split by the mask), then the steps: the states before and after the masked
           reset and after the steps."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from assistive_gym_amd import libagx
from assistive_gym_amd.blob import ModelBlob

mode, out = sys.argv[1], sys.argv[2]
n = int(sys.argv[3]) if len(sys.argv) > 3 else (16 if mode == 'unequal' else 48)
steps = int(sys.argv[4]) if len(sys.argv) > 4 else (20 if mode == 'unequal' else 5)
blob = ModelBlob.load('feeding_jaco')
st = libagx.Stepper(blob, n)
st.reset(seed=4321)
st.synchronize()
s0 = st.get_state()
res = {}
if mode == 'unequal':
    a, b = s0[0].copy(), s0[1].copy()
    blob.view(b[None])['free'][0, :, 0] += 1.0            # every free body of this scene (bowl, food) a metre aside: nothing rests on the spoon, few contacts
    s0 = np.stack([a if i % 2 == 0 else b for i in range(n)])
    st.set_state(s0)
else:
    mask = np.zeros(n, dtype=np.uint8); mask[::3] = 1
    st.reset(mask=torch.from_numpy(mask).cuda(), seed=777)
    st.synchronize()
    s1 = st.get_state()
    keep = mask == 0
    assert np.array_equal(s1[keep].view(np.uint32), s0[keep].view(np.uint32)), 'an environment outside the mask changed'
    assert not np.array_equal(s1[~keep].view(np.uint32), s0[~keep].view(np.uint32))
    res.update(before=s0.view(np.uint32), after_reset=s1.view(np.uint32))
rng = np.random.RandomState(3)
obs_l, rew_l, info_l = [], [], []
for k in range(steps):
    obs, rew, done, info = st.step_host(rng.uniform(-1, 1, (n, blob.act_dim)).astype(np.float32))
    obs_l.append(obs); rew_l.append(rew); info_l.append(info)
res.update(state=st.get_state().view(np.uint32), obs=np.stack(obs_l), reward=np.stack(rew_l), info=np.stack(info_l))
np.savez(out, **res)
if mode == 'unequal':
    rows = np.stack(info_l)[..., 7]
    print('rows per environment (info word 7) at the first step, first four:', rows[0][:4])
    gap = rows[0][0::2].min() - rows[0][1::2].max()
    assert gap >= 30, 'the two scenes of a pair should differ by 30 rows and more (unequal partners): %s' % rows[0][:4]
print('wrote', out, os.environ.get('AGX_LIB', 'libagx.so'))
st.close()
