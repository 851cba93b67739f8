"""Host-side reset for the feeding task (FeedingJaco-v1 and the other robots of model/compiler.py FEEDING_ROBOTS): produces the
pre-settle state record of one environment.  Wheelchair-mounted robots (Jaco, Panda) get Robot.ik_random_restarts from their fixed base;
free-standing ones (Sawyer, Baxter) the base pose search of Robot.position_robot_toc (host/base_pose.py) with the goals
[(target_ee_pos, target_ee_orient)] + [(mouth, None)] (feeding.py:141).

Follows the order of FeedingEnv.reset (assistive_gym/envs/feeding.py:114-182) and what it calls:
build_assistive_env (envs/env.py:114-134: plane friction U(0.025,0.5)), Human.init
(agents/human.py:72-102: gender, impairment, limit scale, strength, tremors), create_human
(human_creation.py:58-66: skin colour draw), head angles U(-30,30)^3 deg (feeding.py:125),
Human.setup_joints (human.py:104-127), target end-effector position (feeding.py:139),
init_robot_pose -> Robot.ik_random_restarts (env.py:276-310, robot.py:84-121), gripper
(feeding.py:144), bowl offset (furniture.py:33), food grid (feeding.py:158-166).

Reset is outside the kernel scope; only its RESULT feeds the stepper.  Seed-level
parity with the reference through reset() is not attainable (the number of RNG draws depends on
Bullet's IK); the draw ORDER up to the IK call is kept.

The 25 settle steps of feeding.py:178-179 are run by the caller on the device (agx_settle).

Unlike the device-side generator (csrc/agx_reset.h, the default everywhere), this numpy sampler does NOT run the collision
rejection of robot.py:105-112 / env.py:299-308: it has no narrowphase of its own.  It is kept as an explicit alternative
(`reset='host'`) for tests and for seeds drawn in the reference's MT19937 order.
"""
import numpy as np

from ..model import xform as X
from .common import (IDENTITY, draw_human, human_model, seated_base, write_human_frames, open_gripper, write_joints, frozen_unless_agent, tool_com_pose,
                     write_env_tail, placement_rng, sample_batch)
from .kin import RobotKin

D = np.deg2rad


class MobilePlacement:
    """init_robot_pose for a robot on wheels (env.py:282-293): the base around toc_base_pos_offset (x, y +- 0.1), its yaw around
    toc_ee_orient_rpy's (+- 30 degrees; none of it in the dressing task), no IK; Stretch.randomize_init_joint_angles (stretch.py:58-62) draws the
    lift height.  The record's base pose is the anchor of the robot's six virtual joints, which start at zero."""

    def __init__(self, blob):
        self.blob, self.kin = blob, RobotKin(blob)
        m = blob.meta
        self.base, self.rpy, self.lift, self.lift_dof = np.array(m['mobile_base'], dtype=np.float64), np.array(m['mobile_rpy'], dtype=np.float64), m['lift'], m['lift_dof']
        self.yaw_range = D(30) if m.get('mobile_yaw', True) else 0.0

    def draw(self, prng):
        """-> base position, base quaternion, joint vector of the robot (virtual joints included)"""
        kin = self.kin
        pos = self.base.copy()
        pos[:2] += prng.uniform(-0.1, 0.1, size=2)
        rpy = self.rpy.copy()
        if self.yaw_range > 0:
            rpy[2] += prng.uniform(-self.yaw_range, self.yaw_range)
        q = np.clip(np.zeros(kin.n), kin.lower, kin.upper)                         # Agent.init -> enforce_joint_limits
        q[self.lift_dof] = self.lift + prng.uniform(-0.1, 0.1)
        return pos, X.quat_from_rpy(rpy), q


def ik_random_restarts(rng, kin, base_pos, base_quat, target_pos, target_quat, max_restarts=1000):
    """Robot.ik_random_restarts (robot.py:84-121) from a fixed base: a random rest pose per restart (the limits randomised after the tenth),
    until the end effector is within 0.01 of the target pose -> (joint vector: the closest one when none qualifies, |position error|, ok, restarts)"""
    ik_lo = np.where(kin.lower < -1e9, -2 * np.pi, kin.lower)                  # agent.py:223-231
    ik_hi = np.where(kin.upper > 1e9, 2 * np.pi, kin.upper)
    best, best_d, ok, restarts = np.clip(np.zeros(kin.n), kin.lower, kin.upper), np.inf, False, 0      # Agent.init -> enforce_joint_limits
    for r in range(max_restarts):
        restarts = r + 1
        lo, hi = ik_lo, ik_hi
        if r >= 10:                                                            # robot.py:91 randomize_limits
            lo = rng.uniform(0, 1, size=kin.n) * ik_lo
            hi = rng.uniform(0, 1, size=kin.n) * ik_hi
        rest = rng.uniform(lo, hi)                                             # agent.py:263
        qs = kin.ik(base_pos, base_quat, rest, target_pos, target_quat, lower=np.minimum(lo, hi), upper=np.maximum(lo, hi))
        qs = np.clip(qs, kin.lower, kin.upper)                                 # set_joint_angles(use_limits=True)
        p, o = kin.ee_pose(base_pos, base_quat, qs)
        dpos = np.linalg.norm(target_pos - p)
        dor = min(np.linalg.norm(target_quat - o), np.linalg.norm(target_quat + o))
        if dpos < best_d:
            best, best_d = qs, dpos
        if dpos < 0.01 and dor < 0.01:                                         # robot.py:97 success_threshold
            best, ok = qs, True
            break
    return best, best_d, ok, restarts


class FeedingJacoReset:
    HEAD_PRESET = [(6, -90), (16, -90), (28, -90), (31, 80), (35, -90), (38, 80)]      # feeding.py:124, drinking.py:132

    def __init__(self, blob):
        self.blob = blob
        self.kin = RobotKin(blob)
        self.base_pos = np.array(blob.meta.get('robot_base_pos', [-0.35, -0.3, 0.36]), dtype=np.float64)
        self.base_quat = np.array(blob.meta.get('robot_base_quat', X.quat_from_rpy([0, 0, -np.pi / 2]).tolist()))
        self.human_bodies = blob.meta.get('human_bodies')
        self.human_dyn = blob.meta.get('human_dynamic_joints', [20, 21, 22, 23])
        self.toc_ee_orient = X.quat_from_rpy(blob.meta.get('ee_rpy', [np.pi / 2.0, 0, np.pi / 2.0]))     # toc_ee_orient_rpy (jaco.py:43)
        self.toc = None
        if blob.meta.get('mount', 'wheelchair') == 'toc':
            from .reset_bed import toc_search
            self.toc = toc_search(blob)
        self.mobile = MobilePlacement(blob) if blob.meta.get('mount') == 'mobile' else None

    def seated_human(self, rng, v, impairment, gender):
        """the draws of build_assistive_env, the seated human with its head angles ~ U(-30, 30)^3 degrees (feeding.py:124-125, drinking.py:132-133),
        its frames in the record, the target at its mouth (feeding.py:184-196) -> (draw, joint angles, target)"""
        b = self.blob
        draw = draw_human(rng, impairment, gender, 4, 20)                          # human.py:89-90 (head joints)
        hm = human_model(draw.gender, draw.limit_scale)
        hq = hm.clamp(np.zeros(hm.n))                                              # human_creation.py:301-314
        for j, a in self.HEAD_PRESET + [(21, rng.uniform(-30, 30)), (22, rng.uniform(-30, 30)), (23, rng.uniform(-30, 30))]:
            hq[j] = D(a)
        hq = hm.clamp(hq)                                                          # set_joint_angles(use_limits) + enforce_joint_limits
        hbase = seated_base(draw.gender)
        hpos, hquat = hm.fk(hbase, IDENTITY, hq)
        write_human_frames(v, self.human_bodies, hpos, hquat, hbase, [0, 0, 0, 1])
        mouth = b.task_f('MOUTH_M' if draw.gender == 'male' else 'MOUTH_F', 3)
        target, _ = X.compose(hpos[23], hquat[23], mouth, IDENTITY)
        return draw, hq, target

    def write_arm_and_head(self, v, draw, hq, q, base_pos, base_quat):
        """gripper, joints (the head: dynamic links, frozen unless the impairment is tremor or the human controllable), the tool in the gripper
        (tool.py:49-62) -> the tool's position"""
        b = self.blob
        open_gripper(b, q)
        write_joints(v, b, q, np.array([hq[j] for j in self.human_dyn]), draw, frozen_unless_agent(b, draw), base_pos, base_quat)
        tp, tq = self.kin.tool_pose(base_pos, base_quat, q)
        free = v['free'][0]
        free[:] = 0
        free[:, 6] = 1.0
        free[b.h['TOOL_BODY'], :3], free[b.h['TOOL_BODY'], 3:7] = tp, tq
        return tp

    def sample(self, rng, state_row, env_seed=0, impairment='random', gender='random', max_restarts=1000, info=None, attempt=0):
        """Fill one state record (float32 view of length state_words) in place.  attempt > 0 (free-standing robots): a re-draw of the
        robot's placement only (init_robot_pose's rejection loop, env.py:281-308)."""
        b, kin = self.blob, self.kin
        v = b.view(state_row)
        draw, hq, target = self.seated_human(rng, v, impairment, gender)
        # robot start pose: IK with random restarts towards a point in front of the person
        target_ee_pos = np.array([-0.15, -0.65, 1.15]) + rng.uniform(-0.05, 0.05, size=3)      # feeding.py:139
        base_pos, base_quat, ok, restarts = self.base_pos, self.base_quat, True, 0
        if self.mobile is not None or self.toc is not None:
            # a robot on wheels (MobilePlacement) or a free-standing one (base pose search).  attempt > 0: init_robot_pose's re-draw after a collision (env.py:299-308)
            prng = placement_rng(np.random.RandomState(rng.randint(1 << 31)), env_seed, attempt)
            if self.mobile is not None:
                base_pos, base_quat, q = self.mobile.draw(prng)
            else:
                base_pos, base_quat, q_arm, _, _ = self.toc.search(prng, target_ee_pos, [target])
                q = np.clip(np.zeros(kin.n), kin.lower, kin.upper)                 # Agent.init -> enforce_joint_limits
                q[self.toc.arm.chain] = q_arm
            best_d = float(np.linalg.norm(target_ee_pos - kin.ee_pose(base_pos, base_quat, q)[0]))
        else:
            q, best_d, ok, restarts = ik_random_restarts(rng, kin, base_pos, base_quat, target_ee_pos, self.toc_ee_orient, max_restarts)
        q = q.copy()
        tp = self.write_arm_and_head(v, draw, hq, q, base_pos, base_quat)          # gripper: feeding.py:144
        free = v['free'][0]
        # bowl on the table (furniture.py:32-34); URDF base frame -> COM frame
        bowl_base = np.array([-0.15, -0.65, 0.75]) + np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0])
        free[1, :3], free[1, 3:7] = tool_com_pose(b, 1, bowl_base, IDENTITY)
        # food grid above the spoon (feeding.py:158-166)
        r_food, k = 0.005, 0
        for i in range(2):
            for j in range(2):
                for kk in range(2):
                    free[b.h['FOOD0'] + k, :3] = np.array([i * 2 * r_food - 0.005, j * 2 * r_food, kk * 2 * r_food + 0.01]) + tp
                    k += 1
        write_env_tail(v, draw, env_seed, b.nfood)
        v['target'][0] = target
        v['food_alive'][0] = (1 << b.nfood) - 1
        v['food_active'][0] = (1 << b.nfood) - 1
        if info is not None:
            info.update(gender=draw.gender, impairment=draw.impairment, limit_scale=draw.limit_scale, strength=draw.strength, tremors=draw.tremors,
                        ik_ok=ok, ik_restarts=restarts, ik_pos_err=best_d, target_ee_pos=target_ee_pos)
        return state_row


FeedingReset = FeedingJacoReset


def make_states(blob, n, seed=1001, impairment='random', checker=None, **kw):
    """n independent post-reset (pre-settle) states; env i uses RandomState(seed + i).  checker(states) -> AGX_COLLIDE_* flags
    (reset_bed.DeviceCollisionChecker): init_robot_pose's collision rejection for the free-standing robots (env.py:281-308)."""
    rs = FeedingJacoReset(blob)
    st = blob.new_state(n)
    infos = [{} for _ in range(n)]
    placed = rs.toc is not None or rs.mobile is not None
    sample_batch(n, seed, lambda i, rng, attempt: rs.sample(rng, st[i:i + 1], env_seed=seed + i, impairment=impairment, info=infos[i], attempt=attempt, **kw),
                 checker if placed else None, infos, st)
    return st, infos
