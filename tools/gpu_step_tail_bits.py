"""GPU box: raw words of a short FeedingJaco rollout for the bit-for-bit comparisons of tests/test_gpu_step_tail.py (one process per library build,
AGX_LIB).  64 environments, 16 copies of each crafted placement of tests/golden/finish_spill_cases.npz (a particle resting on the spoon, in the
shell around SPILL_DIST -- 8 copies on either side --, far away, at the mouth), every copy with random actions of its own, 8 steps; after each
step the observations, rewards, done flags, info words and state records are kept.
usage: AGX_LIB=<build> python tools/gpu_step_tail_bits.py out.npz"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from assistive_gym_amd import libagx
from assistive_gym_amd.blob import ModelBlob

COPIES, STEPS = 16, 8
blob = ModelBlob.load('feeding_jaco')
z = np.load(os.path.join(ROOT, 'tests', 'golden', 'finish_spill_cases.npz'))
rows = [z['resting']] * COPIES + [z['shell_in'], z['shell_out']] * (COPIES // 2) + [z['far']] * COPIES + [z['mouth']] * COPIES
states = np.ascontiguousarray(np.stack(rows), dtype=np.float32)
n = len(states)
st = libagx.Stepper(blob, n)
st.set_state(states)
dev = torch.device('cuda', 0)
obs = torch.zeros((n, blob.obs_dim), dtype=torch.float32, device=dev); rew = torch.zeros(n, dtype=torch.float32, device=dev)
done = torch.zeros(n, dtype=torch.uint8, device=dev); info = torch.zeros((n, 8), dtype=torch.float32, device=dev)
actions = np.random.RandomState(7).uniform(-1, 1, (STEPS, n, blob.act_dim)).astype(np.float32)
actions[0] = 0.0                                 # the placements are made for a first step with a zero action
out = dict(obs=[], reward=[], done=[], info=[], state=[])
s = torch.cuda.current_stream(dev).cuda_stream
for k in range(STEPS):
    st.step_dev(torch.from_numpy(actions[k]).to(dev), obs, rew, done, info, s)
    torch.cuda.synchronize()
    out['obs'].append(obs.cpu().numpy().view(np.uint32)); out['reward'].append(rew.cpu().numpy().view(np.uint32)); out['done'].append(done.cpu().numpy())
    out['info'].append(info.cpu().numpy().view(np.uint32)); out['state'].append(st.get_state().view(np.uint32))
np.savez(sys.argv[1], **{k: np.stack(v) for k, v in out.items()})
st.close()
print('wrote', sys.argv[1], os.environ.get('AGX_LIB', 'libagx.so'))
