"""Host-side reset for ScratchItch<Robot>-v1 / ScratchItch<Robot>Human-v1 (PR2, Sawyer: base pose search; Jaco, Panda: mounted on the
wheelchair): produces post-reset state records (the stepper's input).

Follows the order of ScratchItchEnv.reset (assistive_gym/envs/scratch_itch.py:93-132): build_assistive_env('wheelchair')
(envs/env.py:114-134: plane friction, Human.init draws, agents/human.py:72-102), the seated human with its joint presets
(scratch_itch.py:104-105; Human.setup_joints, human.py:104-127: the right arm stays dynamic -- held by a reactive PD of gain 0.01
and force 1 x strength when the human is not controllable), the target end-effector pose (:115-116), init_robot_pose ->
Robot.position_robot_toc (env.py:276-310, robot.py:123-215) for the base and arm of a free-standing robot, or Robot.ik_random_restarts
(env.py:295-297, robot.py:84-121) from the fixed base of a wheelchair-mounted one (scratch_itch.py:97-99), the gripper (:120), generate_target
(:134-146: limb draw + Util.point_on_capsule, util.py:58-78).

The placement is host/base_pose.py's (BasePoseSearch: Bullet's IK is replaced by damped least squares); the collision rejection loop of
init_robot_pose runs only with a `checker`.
"""
import numpy as np

from ..model import compiler as L
from ..model import xform as X
from .base_pose import BasePoseSearch
from .common import (IDENTITY, draw_human, human_model, seated_base, write_human_frames, open_gripper, write_joints, write_reactive_hold, tool_com_pose,
                     write_env_tail, placement_rng, sample_batch)

D = np.deg2rad


def point_on_limb(rng, radius, length):
    """Util.point_on_capsule (util.py:58-78) for p1 = 0, p2 = (0, 0, -length), theta_range = (0, 2 pi), as generate_target calls it
    (scratch_itch.py:140): two draws, a length along the axis in [radius, length] and an angle."""
    rl = rng.uniform(radius, length)
    th = rng.uniform(0, 2 * np.pi)
    axis, ortho, normal = np.array([0, 0, -1.0]), np.array([0, -1.0, 0]), np.array([-1.0, 0, 0])     # Util.orthogonal_vector of (0, 0, -1)
    return rl * axis + radius * np.cos(th) * ortho + radius * np.sin(th) * normal


def seated_placement(rs, prng, target_ee_pos, goals, wheelchair_yaw, human, **toc_kw):
    """init_robot_pose (env.py:276-310) of a task with a seated human (scratch itch, dressing), by the sampler's mount: a robot on wheels is
    drawn in place, a wheelchair-mounted arm solves IK restarts from its fixed base clear of the human, a free-standing robot searches its base
    pose -> (base position, base quaternion, joint vector, arm angles or None, goals reached, manipulability)"""
    if rs.mount == 'mobile':
        return rs.mobile.draw(prng) + (None, 0, 0.0)
    if rs.mount == 'wheelchair':
        res = rs.search._mounted_ik(prng, target_ee_pos, rs.fixed_base, X.quat_from_rpy([0, 0, wheelchair_yaw]), human=human)
    else:
        res = rs.search.search(prng, target_ee_pos, goals, **toc_kw)
    return res[:2] + (rs.search.arm_joints(res[2]),) + res[2:]


class SeatedReset:
    """what the samplers of the two tasks with a seated human and an arm to reach (scratch itch, dressing) are built from: the mount and its placement"""

    def __init__(self, blob, toc_base, ee_rpy):
        m = blob.meta
        self.blob, self.mount = blob, m.get('mount', 'toc')
        self.arm, self.mobile, self.search = None, None, None
        if self.mount == 'mobile':                                  # the Stretch: no arm chain to solve (env.py:282-293)
            from .reset import MobilePlacement
            self.mobile = MobilePlacement(blob)
        else:
            self.search = BasePoseSearch(blob, toc_base=toc_base, ee_rpy=ee_rpy, self_guard=m.get('robot') == 'sawyer')
            self.arm = self.search.arm
        self.fixed_base = np.array([0, 0, 0.06]) + np.array(m.get('toc_base', [0, 0, 0]))          # wheelchair position + offset (scratch_itch.py:97-99, dressing.py:116-118)

    def seated_human(self, rng, v, impairment, gender, preset, human_q_override, cloth=False):
        """the draws of build_assistive_env, the seated human with the task's joint preset (degrees), its frames in the record
        -> (draw, model, joint angles, link positions, link quaternions, base)"""
        draw = draw_human(rng, impairment, gender, self.blob.nhdof, 10)            # human.py:91-92
        hm = human_model(draw.gender, draw.limit_scale, cloth=cloth)
        hq = hm.clamp(np.zeros(hm.n))                                              # human_creation.py:301-314
        for j, a in preset:
            hq[j] = D(a)
        for j, a in (human_q_override or {}).items():                              # tests only
            hq[j] = a
        hq = hm.clamp(hq)
        hbase = seated_base(draw.gender)
        hpos, hquat = hm.fk(hbase, IDENTITY, hq)
        write_human_frames(v, self.blob.meta['human_bodies'], hpos, hquat, hbase, [0, 0, 0, 1])
        return draw, hm, hq, hpos, hquat, hbase

    def write_robot_and_arm(self, v, draw, hq, q, rb_pos, rb_quat, reactive_gain):
        """gripper, joints; the human's arm stays dynamic: controllable, or held by the reactive PD (reactive_force = 1, human.py:108,124-127)"""
        b = self.blob
        open_gripper(b, q)
        write_joints(v, b, q, np.array([hq[j] for j in b.meta['human_dynamic_joints']]), draw, 0, rb_pos, rb_quat)
        write_reactive_hold(v, b, draw, reactive_gain, 1.0)


class ScratchItchReset(SeatedReset):
    def __init__(self, blob):
        assert blob.task_kind == L.TASK_SCRATCH_ITCH
        SeatedReset.__init__(self, blob, toc_base=[0.1, 0, 0], ee_rpy=[0, 0, 0])  # toc_base_pos_offset (pr2.py:35), toc_ee_orient_rpy (pr2.py:41)

    def sample(self, rng, state_row, env_seed=0, impairment='random', gender='random', info=None, human_q_override=None, attempt=0):
        """attempt > 0: a re-draw of the robot's placement only (init_robot_pose's rejection loop), everything else as on attempt 0"""
        b = self.blob
        v = b.view(state_row)
        preset = [(3, 30), (6, -90), (16, -90), (28, -90), (31, 80), (35, -90), (38, 80)]     # scratch_itch.py:104
        draw, hm, hq, hpos, hquat, hbase = self.seated_human(rng, v, impairment, gender, preset, human_q_override)
        shoulder, elbow, wrist = hpos[5], hpos[7], hpos[9]                         # scratch_itch.py:107-109
        target_ee_pos = np.array([-0.6, 0, 0.8]) + rng.uniform(-0.05, 0.05, size=3)    # scratch_itch.py:115
        prng = placement_rng(np.random.RandomState(rng.randint(1 << 31)), env_seed, attempt)     # one draw of the main stream, whatever the attempt
        rb_pos, rb_quat, q, q_arm, ngoal, manip = seated_placement(self, prng, target_ee_pos, [shoulder, elbow, wrist], -np.pi / 2.0, (hm, hpos, hquat, hbase))   # scratch_itch.py:99
        self.write_robot_and_arm(v, draw, hq, q, rb_pos, rb_quat, 0.01)            # gripper: scratch_itch.py:120; reactive_gain: :105
        tp, tq = self.mobile.kin.tool_pose(rb_pos, rb_quat, q) if q_arm is None else self.search.tool_pose(rb_pos, rb_quat, q_arm)      # tool.py:49-62
        free = v['free'][0]
        free[:] = 0
        free[0, :3], free[0, 3:7] = tool_com_pose(b, 0, tp, tq)
        # generate_target (scratch_itch.py:134-146): limb, then a point on its capsule (util.py:58-78)
        limb = int(rng.randint(2))
        radius, length = hm.dims['upperarm' if limb == 0 else 'forearm']
        target_on_arm = point_on_limb(rng, radius, length)
        task = v['task'][0]
        task[:] = 0
        task[L.SI['TARGET']:L.SI['TARGET'] + 3] = target_on_arm.astype(np.float32).view(np.int32)
        task[L.SI['LIMB']] = limb
        write_env_tail(v, draw, env_seed, 1)                                        # task_success >= 1 x task_success_threshold (scratch_itch.py:37)
        if info is not None:
            info.update(gender=draw.gender, impairment=draw.impairment, limit_scale=draw.limit_scale, strength=draw.strength, tremors=draw.tremors, limb=limb,
                        toc_goals=ngoal, toc_manipulability=manip, target_ee_pos=target_ee_pos, human_q=hq, target_on_arm=target_on_arm)
        return state_row


def make_states(blob, n, seed=1001, impairment='random', checker=None, **kw):
    """n independent post-reset states; env i uses RandomState(seed + i).  checker(states) -> AGX_COLLIDE_* flags
    (reset_bed.DeviceCollisionChecker) turns on init_robot_pose's collision rejection (env.py:281-308)."""
    rs = ScratchItchReset(blob)
    st = blob.new_state(n)
    infos = [{} for _ in range(n)]
    sample_batch(n, seed, lambda i, rng, attempt: rs.sample(rng, st[i:i + 1], env_seed=seed + i, impairment=impairment, info=infos[i], attempt=attempt, **kw),
                 checker, infos, st)
    return st, infos


ScratchItchPR2Reset = ScratchItchReset
