"""GPU box: raw words of a short rollout of one model, for a bit-for-bit comparison of two library builds whose task layer (csrc/agx_task.h: the
observe and finish kernels) must do the same arithmetic (one process per library build, AGX_LIB).  32 environments, 12 steps, a fixed-seed random
action per environment and step; after each step the observations, rewards, done flags, info words and state records are kept.  Start states: the
model's reset pool; bed bathing from bench.wiping_pool (the pad lies on the arm, so wipes happen); dressing with the garments of the host sampler,
as tests/test_gpu_dressing.py sets them; drinking with the water of its pool.  Prints how many (step, environment) entries had a non-zero event
word (AGX_INFO_FOOD_REWARD): a comparison says little about a branch that never ran.
usage: AGX_LIB=<build> python tools/gpu_task_bits.py MODEL[:coop] out.npz;  compare with python tools/gpu_lv_bits.py --compare a.npz b.npz"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from assistive_gym_amd import libagx
from assistive_gym_amd.blob import ModelBlob
from assistive_gym_amd.model import compiler as L
from assistive_gym_amd.vec_env import build_reset_pool

N, STEPS, INFO_EVENT = 32, 12, 4                 # AGX_INFO_FOOD_REWARD (include/agx_blob.h)
model, coop = sys.argv[1].split(':')[0], sys.argv[1].endswith(':coop')
blob = ModelBlob.load(model)
blob = blob.coop() if coop else blob
cloth = None
if blob.task_kind == L.TASK_BED_BATHING:
    import bench
    states = bench.wiping_pool(blob, N, 1001)
elif blob.task_kind == L.TASK_DRESSING:
    from assistive_gym_amd.host.reset_dressing import make_states
    states, cloth, _ = make_states(blob, N, seed=9001)
else:
    states = build_reset_pool(blob, N, seed=1001)
    if isinstance(states, tuple):
        states, cloth = states
states = np.ascontiguousarray(states, dtype=np.float32)
st = libagx.Stepper(blob, N)
st.set_state(states)
if cloth is not None:
    st.set_cloth(cloth)
dev = torch.device('cuda', 0)
obs = torch.zeros((N, blob.obs_dim), dtype=torch.float32, device=dev); rew = torch.zeros(N, dtype=torch.float32, device=dev)
done = torch.zeros(N, dtype=torch.uint8, device=dev); info = torch.zeros((N, 8), dtype=torch.float32, device=dev)
actions = np.random.RandomState(11).uniform(-1, 1, (STEPS, N, blob.act_dim)).astype(np.float32)
out = dict(obs=[], reward=[], done=[], info=[], state=[])
s = torch.cuda.current_stream(dev).cuda_stream
for k in range(STEPS):
    st.step_dev(torch.from_numpy(actions[k]).to(dev), obs, rew, done, info, s)
    torch.cuda.synchronize()
    out['obs'].append(obs.cpu().numpy().view(np.uint32)); out['reward'].append(rew.cpu().numpy().view(np.uint32)); out['done'].append(done.cpu().numpy())
    out['info'].append(info.cpu().numpy().view(np.uint32)); out['state'].append(st.get_state().view(np.uint32))
res = {k: np.stack(v) for k, v in out.items()}
np.savez(sys.argv[2], start=states.view(np.uint32), **res)
st.close()
events = int((res['info'][:, :, INFO_EVENT].view(np.float32) != 0).sum())
print('wrote %s %s %s: %d of %d (step, environment) entries with a non-zero event word' % (sys.argv[2], sys.argv[1], os.environ.get('AGX_LIB', 'libagx.so'), events, STEPS * N))
