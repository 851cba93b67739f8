"""GPU box: raw words of a short rollout from the reset pool for the bit-for-bit comparison of tests/test_gpu_face_proof.py (one process per library
build, AGX_LIB).  Random actions; after each step the observations, rewards, done flags, info words and state records are kept, and of the first
step the debug record of its first substep: head words (contact and row counts), contact records, inverse mass matrix, accelerations (not the
cycle counters, and not the copy of the scratch record's row area, which is only defined up to the rows of that substep).
usage: AGX_LIB=<build> python tools/gpu_face_proof_bits.py <model> <environments> <steps> out.npz"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from assistive_gym_amd import libagx
from assistive_gym_amd.blob import ModelBlob
from assistive_gym_amd.vec_env import build_reset_pool

model, n, steps, path = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
blob = ModelBlob.load(model)
states = np.ascontiguousarray(build_reset_pool(blob, n, seed=2024), dtype=np.float32)
st = libagx.Stepper(blob, n)
st.set_state(states)
dev = torch.device('cuda', 0)
obs = torch.zeros((n, blob.obs_dim), dtype=torch.float32, device=dev); rew = torch.zeros(n, dtype=torch.float32, device=dev)
done = torch.zeros(n, dtype=torch.uint8, device=dev); info = torch.zeros((n, 8), dtype=torch.float32, device=dev)
words, o_con, o_minv, _, o_hdr, _, _, o_qdd = st.debug_layout()
debug = torch.zeros((n, words), dtype=torch.float32, device=dev)
actions = np.random.RandomState(11).uniform(-1, 1, (steps, n, blob.act_dim)).astype(np.float32)
out = dict(pool=[states.view(np.uint32)], obs=[], reward=[], done=[], info=[], state=[])
s = torch.cuda.current_stream(dev).cuda_stream
for k in range(steps):
    st.step_dev(torch.from_numpy(actions[k]).to(dev), obs, rew, done, info, s, debug=debug if k == 0 else None)
    torch.cuda.synchronize()
    if k == 0:
        d = debug.cpu().numpy()
        ncon = d[:, 0].astype(np.int64)
        con = d[:, o_con:o_minv].reshape(n, -1, 16).copy()
        con[np.arange(con.shape[1])[None, :] >= ncon[:, None]] = 0.0          # slots beyond the substep's contacts
        out['debug'] = [np.concatenate([d[:, :16], con.reshape(n, -1), d[:, o_minv:o_hdr], d[:, o_qdd:]], axis=1).view(np.uint32)]
    out['obs'].append(obs.cpu().numpy().view(np.uint32)); out['reward'].append(rew.cpu().numpy().view(np.uint32)); out['done'].append(done.cpu().numpy())
    out['info'].append(info.cpu().numpy().view(np.uint32)); out['state'].append(st.get_state().view(np.uint32))
np.savez(path, **{k: np.stack(v) for k, v in out.items()})
st.close()
print('wrote', path, model, n, steps, os.environ.get('AGX_LIB', 'libagx.so'))
