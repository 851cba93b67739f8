"""Host-side reset for DressingBaxter-v1 / DressingBaxterHuman-v1: post-reset state records and garments (the stepper's input).

Follows the order of DressingEnv.reset (assistive_gym/envs/dressing.py:112-198): build_assistive_env('wheelchair_left')
(envs/env.py:114-134: plane friction, Human.init draws, agents/human.py:72-102), motor gains 0.01 (:121), the seated human with
both elbows bent and the left shoulder abducted (:123-124; its left arm stays dynamic, held by a reactive PD of gain 0.01 and
force 1 x strength when the human is not controllable), the target end-effector pose (:130-133), init_robot_pose ->
Robot.position_robot_toc on the human's LEFT (right_side=False: env.py:298, robot.py:143) with oriented goals 10 cm above the
shoulder, elbow and wrist (:134), the gripper (:140), the garment loaded relative to the end effector (:146-153: every node is
shifted by cloth_offset = start_ee_pos - cloth_orig_pos) and hung from the massless attachment sphere at the end effector,
gravity -9.81 / 2 on the cloth while 50 simulation steps let it settle (:178-192), then -9.81.

The 50-step settle needs the stepper: `settler` advances (state records, garments) by n stepSimulation calls -- ClothSettler runs
it on the device (agx_settle); tests pass an oracle-backed one.  The mount and its placement are host/reset_scratch.py's SeatedReset over
host/base_pose.py (Bullet's IK is replaced by damped least squares; Baxter's half_range IK limits, baxter.py:49, are not modelled);
init_robot_pose's collision loop runs only with a `checker`.
"""
import numpy as np

from ..model import compiler as L
from ..model import xform as X
from .common import DeviceBatch, write_env_tail, placement_rng, sample_batch
from .reset_scratch import SeatedReset, seated_placement

D = np.deg2rad


def cloth_x0(blob):
    """node positions of the garment for cloth_offset = 0 (float64 [NN, 3])"""
    oc = blob.h['OFF_CLOTH']
    nn = int(blob.i[oc + L.CL['NN']])
    o = oc + int(blob.i[oc + L.CL['OFF_X0']])
    return blob.f[o:o + 3 * nn].reshape(nn, 3).astype(np.float64)


def cloth_nodes(blob):
    return int(blob.i[blob.h['OFF_CLOTH'] + L.CL['NN']])


class DressingReset(SeatedReset):
    def __init__(self, blob):
        assert blob.task_kind == L.TASK_DRESSING
        SeatedReset.__init__(self, blob, toc_base=[1.7, 0.7, 0.925], ee_rpy=[0, -np.pi / 2.0, 0])        # toc_base_pos_offset (baxter.py:39), toc_ee_orient_rpy['dressing'][0] (baxter.py:45)
        self.ee_R_shoulder = X.quat_to_mat(X.quat_from_rpy(blob.meta.get('ee_rpy_shoulder', [np.pi / 2.0, -np.pi / 2.0, 0])))   # [-1]
        self.x0 = cloth_x0(blob)
        self.cloth_orig_pos = np.array(blob.meta['cloth_orig_pos'])

    def sample(self, rng, state_row, cloth_row, env_seed=0, impairment='random', gender='random', info=None, human_q_override=None, attempt=0):
        """Fill one state record and one garment (float32 [2, NN, 3]: positions, velocities) in place -- BEFORE the cloth has settled;
        the record's cloth gravity is the settle value -9.81 / 2 (dressing.py:178)."""
        b = self.blob
        v = b.view(state_row)
        preset = [(6, -90), (13, -45), (16, -90), (28, -90), (31, 80), (35, -90), (38, 80)]     # dressing.py:123
        draw, hm, hq, hpos, hquat, hbase = self.seated_human(rng, v, impairment, gender, preset, human_q_override, cloth=True)
        shoulder, elbow, wrist = hpos[15], hpos[17], hpos[19]                      # left shoulder / elbow / wrist (dressing.py:126-128)
        target_ee_pos = np.array([0.45, -0.3, 1]) + rng.uniform(-0.05, 0.05, size=3)    # dressing.py:130
        off = np.array([0, 0, 0.1])
        prng = placement_rng(rng, env_seed, attempt)     # attempt > 0: a re-draw of the placement only (env.py:281); nothing else is drawn after it
        # on the human's LEFT: the wheelchair-mounted arm's base is turned by pi / 2 (env.py:295-297), the free-standing robot's drawn left of the human
        ee_R = None if self.search is None else self.search.ee_R
        rb_pos, rb_quat, q, q_arm, ngoal, manip = seated_placement(self, prng, target_ee_pos, [shoulder + off, elbow + off, wrist + off], np.pi / 2.0, (hm, hpos, hquat, hbase),
                                                                   goal_Rs=[self.ee_R_shoulder, ee_R, ee_R], right_side=False)
        self.write_robot_and_arm(v, draw, hq, q, rb_pos, rb_quat, 0.01)            # gripper: dressing.py:140; reactive_gain: :124
        if q_arm is None:
            start_ee_pos = self.mobile.kin.ee_pose(rb_pos, rb_quat, q)[0]
        else:
            start_ee_pos = self.arm.fk(rb_pos[None], X.quat_to_mat(rb_quat)[None], q_arm[None])[0][0]      # dressing.py:146
        cloth_offset = start_ee_pos - self.cloth_orig_pos                          # :148-149
        cloth_row[0] = (self.x0 + cloth_offset).astype(np.float32)
        cloth_row[1] = 0
        task = v['task'][0]
        task[:] = 0
        task[L.DR['CLOTH_GRAVITY']:L.DR['CLOTH_GRAVITY'] + 1] = np.array([-9.81 / 2], dtype=np.float32).view(np.int32)    # :178
        write_env_tail(v, draw, env_seed, 1)
        if info is not None:
            info.update(gender=draw.gender, impairment=draw.impairment, limit_scale=draw.limit_scale, strength=draw.strength, tremors=draw.tremors,
                        toc_goals=ngoal, toc_manipulability=manip, target_ee_pos=target_ee_pos, human_q=hq, start_ee_pos=start_ee_pos)
        return state_row


def finish_settle(blob, states):
    """after the settle: full gravity on the cloth (dressing.py:195), velocities of the articulated bodies as they are"""
    v = blob.view(states)
    v['task'][:, L.DR['CLOTH_GRAVITY']] = np.array([-9.81], dtype=np.float32).view(np.int32)[0]
    v['iteration'][:] = 0
    return states


class ClothSettler(DeviceBatch):
    """Runs the 50-step cloth settle of DressingEnv.reset on the device (agx_settle on the dressing model with the garments attached)."""

    def __call__(self, states, cloth, n_sim_steps):
        return self.settle(states, n_sim_steps, cloth)


def make_states(blob, n, seed=1001, impairment='random', settler=None, settle_steps=50, checker=None, **kw):
    """n independent post-reset (state record, garment) pairs; env i uses RandomState(seed + i).  settler(states, cloth, n_sim_steps)
    -> (states, cloth) runs the cloth settle (ClothSettler: on the device); without one the garment is left as loaded."""
    rs = DressingReset(blob)
    st = blob.new_state(n)
    cloth = np.zeros((n, 2, cloth_nodes(blob), 3), dtype=np.float32)
    infos = [{} for _ in range(n)]
    sample_batch(n, seed, lambda i, rng, attempt: rs.sample(rng, st[i:i + 1], cloth[i], env_seed=seed + i, impairment=impairment, info=infos[i], attempt=attempt, **kw),
                 checker, infos, st)          # init_robot_pose's collision rejection (env.py:281-308): before the garment settles
    if settler is not None:
        st, cloth = settler(st, cloth, settle_steps)
    return finish_settle(blob, st), cloth, infos


DressingBaxterReset = DressingReset
