"""Host-side reset for DrinkingJaco-v1 (MODEL + CPU ORACLE ONLY so far: no kernel variant serves the drinking task): the pre-settle
state record and the water buffer of one environment.

Follows the order of DrinkingEnv.reset (assistive_gym/envs/drinking.py:123-181): build_assistive_env('wheelchair') (env.py:114-134), the
mounted robot on the wheelchair (:126-128), motor gains 0.005 (:130), the seated human with the head draws (:132-134), generate_target
(:183-196), the cup in the gripper (:137, tool.py:49-62), target_ee_pos around [-0.2, -0.5, 1.1] and Robot.ik_random_restarts (:141-143,
env.py:295-297), the gripper (:146), the 4 x 4 x 4 grid of water spheres above the cup's base frame (:160-167).  The 50 settle steps of
:176-177 are the caller's (oracle: settle_cloth).  As in host/reset.py: Bullet's IK is replaced by damped least squares; no collision
rejection here.
"""
import numpy as np

from ..model import compiler as L
from .common import write_env_tail, sample_batch
from .reset import FeedingJacoReset, ik_random_restarts

D = np.deg2rad


def water_x0(blob):
    """rest offsets of the particles relative to the cup's base frame position (the section's X0)"""
    oc = blob.h['OFF_CLOTH']
    nn = int(blob.i[oc + L.CL['NN']])
    o = oc + int(blob.i[oc + L.CL['OFF_X0']])
    return blob.f[o:o + 3 * nn].reshape(nn, 3).astype(np.float64)


class DrinkingReset(FeedingJacoReset):
    def __init__(self, blob):
        assert blob.task_kind == L.TASK_DRINKING
        FeedingJacoReset.__init__(self, blob)
        self.x0 = water_x0(blob)

    def sample(self, rng, state_row, water_row, env_seed=0, impairment='random', gender='random', max_restarts=1000, info=None):
        b, kin = self.blob, self.kin
        v = b.view(state_row)
        draw, hq, target = self.seated_human(rng, v, impairment, gender)           # drinking.py:132-134, :190-196
        target_ee_pos = np.array([-0.2, -0.5, 1.1]) + rng.uniform(-0.05, 0.05, size=3)          # drinking.py:141
        q, best_d, ok, restarts = ik_random_restarts(rng, kin, self.base_pos, self.base_quat, target_ee_pos, self.toc_ee_orient, max_restarts)
        q = q.copy()
        tp = self.write_arm_and_head(v, draw, hq, q, self.base_pos, self.base_quat)      # gripper: drinking.py:146; the cup: tool.py:49-62
        water_row[0] = (self.x0 + tp).astype(np.float32)                           # drinking.py:163-167: the grid is added to cup_pos, world axes
        water_row[1] = 0
        write_env_tail(v, draw, env_seed, len(self.x0))                            # total_water_count (drinking.py:171)
        v['target'][0] = target
        task = v['task'][0]
        task[:] = 0
        task[L.DK['ALIVE']:L.DK['ALIVE'] + 2] = -1                                 # self.waters / self.waters_active: all 64 (drinking.py:168-172)
        task[L.DK['ACTIVE']:L.DK['ACTIVE'] + 2] = -1
        if info is not None:
            info.update(gender=draw.gender, impairment=draw.impairment, limit_scale=draw.limit_scale, strength=draw.strength, tremors=draw.tremors, ik_ok=ok,
                        ik_restarts=restarts, ik_pos_err=best_d, target_ee_pos=target_ee_pos, cup_pos=tp)
        return state_row


def make_states(blob, n, seed=1001, impairment='random', **kw):
    """n independent pre-settle states and their water buffers (float32 [n, 2, 64, 3]); env i uses RandomState(seed + i)"""
    rs = DrinkingReset(blob)
    st = blob.new_state(n)
    water = np.zeros((n, 2, len(rs.x0), 3), dtype=np.float32)
    infos = [{} for _ in range(n)]
    sample_batch(n, seed, lambda i, rng, attempt: rs.sample(rng, st[i:i + 1], water[i], env_seed=seed + i, impairment=impairment, info=infos[i], **kw), None, infos, st)
    return st, water, infos
