"""Host-side reset for ArmManipulationSawyer-v1 / ArmManipulationSawyerHuman-v1: post-reset state records (the stepper's input).

Follows the order of ArmManipulationEnv.reset (assistive_gym/envs/arm_manipulation.py:110-182): build_assistive_env('bed',
fixed_human_base=False, human_impairment='no_tremor') (envs/env.py:114-134), motor forces 20 / 2 (:114-115), the posed human dropped
from [-0.25, 0.2, 0.95] as a rag doll for 100 simulation steps at gravity -1 onto the bed at friction 5 (:117-134), bed friction 0.3
(:136), the right arm posed at shoulder (60, -60) degrees / elbow 0 and left dynamic while every other link becomes static
(:139-142; a reactive hold of 0.01 N m x strength, gain 0.05), 100 more simulation steps in which the arm falls beside the body
(:145-146), the target end-effector poses (:158-159: both are drawn), init_robot_pose -> Robot.position_robot_toc with the goals wrist,
waist, elbow, stomach (:162), the scooper in the gripper (:154,173), gravity -9.81 with none on the tool (:176-177).

Both settles need the stepper: `settler` is the rag-doll settle of host/reset_bed.py (RagdollSettler), `arm_settler` advances
arm-manipulation state records by n stepSimulation calls at gravity -1 (ArmFallSettler: on the device, the robot and its tool parked
out of reach); tests pass oracle-backed ones.  The sampler holds a BasePoseSearch (host/base_pose.py: Bullet's IK is replaced by damped least
squares) and a BedSurface (host/reset_bed.py) of its own; init_robot_pose's collision loop runs only with a `checker`.
"""
import numpy as np

from ..model import compiler as L
from .base_pose import BasePoseSearch
from .common import DeviceBatch, IDENTITY, draw_of, write_human_frames, open_gripper, tool_com_pose, write_env_tail, placement_rng, flag_collisions
from .reset_bed import BedSurface, pose_in_air, rest_on_bed

D = np.deg2rad
PARKED = np.array([20.0, 20.0, 0.975])          # where the robot stands while the arm falls (it is not yet placed then, :162)


class ArmManipulationSawyerReset:
    def __init__(self, blob):
        assert blob.task_kind == L.TASK_ARM_MANIPULATION
        self.blob = blob
        self.dual = bool(blob.meta.get('dual'))          # a two-armed robot: tool_right in the right hand (self.arm), tool_left in the left (self.arm2)
        # toc_base_pos_offset (sawyer.py:40), toc_ee_orient_rpy (sawyer.py:46)
        self.search = BasePoseSearch(blob, toc_base=[-0.3, 0.6, 0.975], ee_rpy=[0, -np.pi / 2.0, np.pi], self_guard=blob.meta.get('robot', 'sawyer') == 'sawyer', dual=self.dual)
        self.arm, self.arm2 = self.search.arm, self.search.arm2
        self.bed = BedSurface(blob)

    def pre_settle(self, rng, impairment='no_tremor', gender='random', human_q_override=None):
        return pose_in_air(rng, self.blob, impairment, gender, human_q_override, [-0.25, 0.2, 0.95])      # arm_manipulation.py:123

    def _place(self, v, rb_pos, rb_quat, q_arm, q_arm2=None):
        """robot joints, base and the tool(s) in the gripper(s) (tool.py:49-62)"""
        b, nr = self.blob, self.blob.nrobot
        q = open_gripper(b, self.search.arm_joints(q_arm, q_arm2))                 # :170
        v['q'][0, :nr] = q
        v['qd'][0, :nr] = 0
        v['qt'][0, :nr] = q
        v['base'][0, :3], v['base'][0, 3:] = rb_pos, rb_quat
        free = v['free'][0]
        free[:] = 0
        free[0, :3], free[0, 3:7] = tool_com_pose(b, 0, *self.search.tool_pose(rb_pos, rb_quat, q_arm))
        if self.dual:
            free[1, :3], free[1, 3:7] = tool_com_pose(b, 1, *self.search.tool_pose(rb_pos, rb_quat, q_arm2, second=True))

    def arm_fall_record(self, state_row, pre, env_seed=0):
        """the record the second settle starts from (:136-142): the human resting, its right arm posed, the robot parked"""
        b = self.blob
        v = b.view(state_row)
        state_row[:] = 0
        nr = b.nrobot
        hm, hq = pre['hm'], pre['hq']
        hq = hq.copy()
        hq[3], hq[4], hq[6] = D(60), D(-60), 0.0                                   # j_right_shoulder_x / _y, j_right_elbow (:139)
        hq = hm.clamp(hq)                                                          # enforce_joint_limits (human.py:121)
        pre['hq'] = hq
        write_human_frames(v, b.meta['human_bodies'], *hm.fk(pre['base_pos'], pre['base_quat'], hq), pre['base_pos'], pre['base_quat'])
        mid = [np.where((a.lower > -1e9) & (a.upper < 1e9), 0.5 * (a.lower + a.upper), 0.0) for a in (self.arm, self.arm2) if a is not None]
        self._place(v, PARKED, IDENTITY, *mid)            # parked at the middle of its joint ranges (the Jaco's zero pose violates its limits)
        hq_dyn = np.array([hq[j] for j in b.meta['human_dynamic_joints']])
        v['q'][0, nr:] = hq_dyn
        v['qt'][0, nr:] = hq_dyn
        v['qd'][0, nr:] = 0
        v['tremor'][0] = 0
        v['tremor_target'][0] = hq_dyn                                             # human.py:123 target_joint_angles
        v['frozen'][0] = 0                                                         # the right arm is dynamic in every episode
        # the reactive hold of setup_joints (:140, human.py:124-127); a controllable human's motors are re-targeted by every take_step
        v['human_kp'][0] = 0.0 if b.is_coop else 0.05
        v['human_maxf'][0] = 0.0 if b.is_coop else 0.01 * pre['strength']
        v['limit_scale'][0] = pre['limit_scale']
        write_env_tail(v, draw_of(pre), env_seed, 1)
        return state_row

    def post_fall(self, rng, state_row, pre, env_seed=0, info=None, attempt=0):
        """everything after the arm has fallen (:148-179); the record keeps the arm's joint angles AND velocities"""
        b = self.blob
        v = b.view(state_row)
        nr = b.nrobot
        hm, hq = pre['hm'], pre['hq'].copy()
        for k, j in enumerate(b.meta['human_dynamic_joints']):
            hq[j] = v['q'][0, nr + k]
        hpos, _ = hm.fk(pre['base_pos'], pre['base_quat'], hq)
        elbow, wrist, stomach, waist = hpos[7], hpos[9], hpos[24], hpos[27]        # :148-151
        if attempt == 0:
            pre['target_ee_pos'] = np.array([-1, -0.3 if self.dual else 0.4, 0.8]) + rng.uniform(-0.05, 0.05, size=3)    # :158
            pre['target_ee_left_pos'] = np.array([-1, 0.7, 0.8]) + rng.uniform(-0.05, 0.05, size=3)                    # :159 (drawn for a single arm as well)
        target_ee_pos = pre['target_ee_pos']
        prng = placement_rng(rng, env_seed, attempt)
        if self.dual:     # :165: the right arm's goals are wrist and waist, the left arm's elbow and stomach
            rb_pos, rb_quat, (q_arm, q_arm2), ngoal, manip = self.search.search_dual(prng, [target_ee_pos, pre['target_ee_left_pos']], [[wrist, waist], [elbow, stomach]])
        else:
            rb_pos, rb_quat, q_arm, ngoal, manip = self.search.search(prng, target_ee_pos, [wrist, waist, elbow, stomach])   # :162
            q_arm2 = None
        self._place(v, rb_pos, rb_quat, q_arm, q_arm2)
        v['iteration'][0] = 0
        v['task_success'][0] = 0
        v['task'][0] = 0                                                           # AM_BEST: task_success = 0 (init_env_variables)
        if info is not None:
            info.update(gender=pre['gender'], impairment=pre['impairment'], limit_scale=pre['limit_scale'], strength=pre['strength'],
                        toc_goals=ngoal, toc_manipulability=manip, target_ee_pos=target_ee_pos, human_q=hq, human_base=(pre['base_pos'], pre['base_quat']))
        return state_row


class ArmFallSettler(DeviceBatch):
    """Runs the second settle of ArmManipulationEnv.reset on the device: agx_settle on the arm-manipulation model with the human's gravity
    set to the reset's -1 (arm_manipulation.py:125,145-146)."""

    def __init__(self, blob, n_envs, device=0):
        DeviceBatch.__init__(self, blob.set_param('HUMAN_GRAVITY_Z', -1.0), n_envs, device)

    def __call__(self, states, n_sim_steps):
        return self.settle(states, n_sim_steps)


def make_states(blob, n, seed=1001, impairment='no_tremor', settler=None, arm_settler=None, fall_steps=100, checker=None, **kw):
    """n independent post-reset states; env i uses RandomState(seed + i).  settler: bed_settle records -> records after the 100-step
    rag-doll settle (host/reset_bed.RagdollSettler; None = the rigid 'drop' stand-in); arm_settler(states, n_sim_steps): the arm's fall
    (ArmFallSettler; None = the arm stays as posed); checker(states) -> AGX_COLLIDE_* flags (reset_bed.DeviceCollisionChecker) turns on
    init_robot_pose's collision rejection (env.py:281-308)."""
    rs = ArmManipulationSawyerReset(blob)
    st = blob.new_state(n)
    infos = [{} for _ in range(n)]
    rngs = [np.random.RandomState(seed + i) for i in range(n)]
    pres = [rs.pre_settle(rngs[i], impairment=impairment, **kw) for i in range(n)]
    if settler is None:
        for p in pres:
            p['base_pos'] = rs.bed.drop(p['hm'], p['base_pos'], p['base_quat'], p['hq'])
    else:
        rest_on_bed(settler, pres)
    for i, p in enumerate(pres):
        rs.arm_fall_record(st[i:i + 1], p, env_seed=seed + i)
    if arm_settler is not None:
        st = np.ascontiguousarray(arm_settler(st, fall_steps))

    def place(i, attempt=0):
        rs.post_fall(rngs[i], st[i:i + 1], pres[i], env_seed=seed + i, info=infos[i], attempt=attempt)
    for i in range(n):
        place(i)
    flag_collisions(st, checker, place, infos)
    return st, infos
