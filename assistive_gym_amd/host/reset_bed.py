"""Host-side reset for BedBathingSawyer-v1: produces post-reset state records (the stepper's input).

Follows the order of BedBathingEnv.reset (assistive_gym/envs/bed_bathing.py:112-171) and what it calls:
build_assistive_env('bed', fixed_human_base=False) (envs/env.py:114-134: plane friction, Human.init draws,
agents/human.py:72-102), the human posed in the air and its joints perturbed by U(-0.1, 0.1) (bed_bathing.py:119-127),
the settle onto the bed (bed_bathing.py:129-137), the target end-effector pose (bed_bathing.py:147-148),
init_robot_pose -> Robot.position_robot_toc (env.py:276-310, robot.py:123-215: 50 random base poses scored by goals
reached and joint-limit-weighted kinematic isotropy), the gripper (bed_bathing.py:156), generate_targets
(bed_bathing.py:173-188) and the per-body gravities (bed_bathing.py:160-165, compiled into the blob).

Reset is outside the kernel scope; only its RESULT feeds the stepper.  What is NOT the reference's:
  * Bullet's IK is replaced by damped least squares (as in host/kin.py); the TOC search keeps the reference's structure
    (50 attempts, start pose + 3 position-only goals, success threshold 0.03, JLWKI score);
  * the 100-step rag-doll settle of the 47-DoF floating human (bed_bathing.py:129-131) is produced by `settle`:
    'ragdoll' runs it: the bed_settle model (compiler.compile_bed_settle: the human as one floating articulated body, its own
    kernel variant) is stepped 100 times by a `settler` (RagdollSettler: the device, through agx_settle) and the resting base
    pose and joint angles are read back; 'drop' (the default without a device) lowers the posed human rigidly until its first
    collider touches the mattress -- a kinematic stand-in that keeps the perturbed joint angles but lets limbs float above
    the bed by the difference of their radii;
  * the collision rejection loop of init_robot_pose (env.py:299-308) runs only with a `checker` (DeviceCollisionChecker).

The base pose search is host/base_pose.py's (BasePoseSearch), the draws and writers every sampler shares are host/common.py's; this module
also holds the rag-doll records and settler and the bed's surface (BedSurface), which the arm-manipulation sampler uses too.
"""
import numpy as np

from ..model import compiler as L
from ..model import xform as X
from .base_pose import ArmChain, BasePoseSearch      # noqa: F401 (ArmChain: imported from here by tests and tools)
from .common import (DeviceBatch, draw_human, draw_of, human_model, write_human_frames, open_gripper, write_joints, frozen_unless_agent, tool_com_pose, write_env_tail,
                     placement_rng, reject_collisions, flag_collisions)      # noqa: F401 (reject_collisions: imported from here by tests)

D = np.deg2rad


def settle_record(sblob, row, gender, limit_scale, base_pos, base_rpy, hq, plane_friction):
    """state record of the bed_settle model: the posed human in the air (bed_bathing.py:121,127), at rest"""
    v = sblob.view(row)
    row[:] = 0
    joints = sblob.meta['settle_joints']
    q = np.concatenate([base_pos, [base_rpy[2], base_rpy[1], base_rpy[0]], [hq[j] for j in joints]])
    v['q'][0] = q
    v['qt'][0] = q
    v['human'][0, 0, 3:] = [0, 0, 0, 1]                       # the world anchor of the virtual root joints
    v['base'][0, 3:] = [0, 0, 0, 1]
    v['limit_scale'][0] = limit_scale
    v['plane_friction'][0] = plane_friction
    v['gender'][0] = 0 if gender == 'male' else 1
    return row


def settled_pose(sblob, row, hm):
    """(base_pos, base_quat, hq[hm.n]) of a settle record"""
    v = sblob.view(row)
    q = v['q'][0].astype(np.float64)
    hq = np.zeros(hm.n)
    for k, j in enumerate(sblob.meta['settle_joints']):
        hq[j] = q[6 + k]
    return q[:3].copy(), X.quat_from_rpy([q[5], q[4], q[3]]), hq


class RagdollSettler(DeviceBatch):
    """Runs the rag-doll settle on the device: an agx context on the bed_settle model, agx_settle for 100 simulation steps
    (bed_bathing.py:130-131)."""

    def __init__(self, n_envs, device=0, steps=100):
        from ..blob import ModelBlob
        DeviceBatch.__init__(self, ModelBlob.load('bed_settle'), n_envs, device)
        self.steps = steps

    def __call__(self, states):
        return self.settle(states, self.steps)


class DeviceCollisionChecker(DeviceBatch):
    """states -> AGX_COLLIDE_* flags per state, from the stepper's own collision pass on the device (agx_check_collisions): the
    collision rejection of init_robot_pose / ik_random_restarts (env.py:299-308, robot.py:103-108) for resets sampled on the host."""

    def __call__(self, states):
        out = np.zeros(len(states), dtype=np.uint8)
        for i0 in range(0, len(states), self.n):
            chunk = states[i0:i0 + self.n]
            self.load(chunk)
            out[i0:i0 + len(chunk)] = self.ctx.check_collisions()[:len(chunk)]
        return out


def toc_search(blob):
    """the base pose search for a task whose blob states the robot's toc_base and ee_rpy itself (feeding)"""
    return BasePoseSearch(blob, self_guard=blob.meta.get('robot') == 'sawyer')


def rest_on_bed(settler, pres):
    """the rag-doll settle of a batch (bed_bathing.py:129-137): the posed humans of `pres` (pre_settle) as bed_settle records through `settler`;
    their resting base pose and joint angles replace the posed ones"""
    from ..blob import ModelBlob
    sblob = settler.blob if hasattr(settler, 'blob') else ModelBlob.load('bed_settle')
    ss = sblob.new_state(len(pres))
    for i, p in enumerate(pres):
        settle_record(sblob, ss[i:i + 1], p['gender'], p['limit_scale'], p['base_pos'], p['base_rpy'], p['hq'], p['plane_friction'])
    ss = settler(ss)
    for i, p in enumerate(pres):
        p['base_pos'], p['base_quat'], p['hq'] = settled_pose(sblob, ss[i:i + 1], p['hm'])


class BedSurface:
    """the bed's collision geometry as the rigid 'drop' stand-in for the rag-doll settle sees it"""

    def __init__(self, blob):
        self._bed = [blob.collider(c)['verts'] for c in range(*blob.meta['ranges']['bed'])]
        self._bed_box = np.array([[v.min(0), v.max(0)] for v in self._bed])

    def top(self, x, y):
        """height of the bed's collision geometry under (x, y): top of the hulls whose footprint box contains the point"""
        b = self._bed_box
        inside = (b[:, 0, 0] <= x) & (x <= b[:, 1, 0]) & (b[:, 0, 1] <= y) & (y <= b[:, 1, 1]) & (b[:, 1, 2] < 0.9)   # not the head / foot boards
        return float(b[inside, 1, 2].max()) + L.HULL_MARGIN if inside.any() else 0.0

    def drop(self, hm, base_pos, base_quat, hq):
        """lowers the rigidly posed human until its first collider rests on the bed"""
        pos, quat = hm.fk(base_pos, base_quat, hq)
        dz = -np.inf
        for link, kind, data in hm.colliders():
            lp, lq = (base_pos, base_quat) if link < 0 else (pos[link], quat[link])
            if kind == 'capsule':
                pts, r = X.apply(lp, lq, np.stack([data[0], data[1]])), data[2]
            elif kind == 'sphere':
                pts, r = X.apply(lp, lq, data[0][None]), data[1]
            else:
                continue            # the head mesh: it rests on the pillow region, the neck / chest decide
            for p in pts:
                dz = max(dz, self.top(p[0], p[1]) + r - p[2])
        return base_pos + np.array([0, 0, dz])


def pose_in_air(rng, blob, impairment, gender, human_q_override, base_pos):
    """the draws of build_assistive_env and the posed human in the air (bed_bathing.py:114-127; arm_manipulation.py:112-127 from another spot)"""
    draw = draw_human(rng, impairment, gender, blob.nhdof, 10)                 # human.py:91-92 (the head is not controllable)
    hm = human_model(draw.gender, draw.limit_scale)
    # bed_bathing.py:119-127: pose in the air, every motor joint ~ U(-0.1, 0.1) (this overwrites the 30 degree shoulder preset), limits enforced
    hq = np.zeros(hm.n)
    movable = [j for j in range(hm.n) if hm.jtype[j] == 'r']
    hq[movable] = rng.uniform(-0.1, 0.1, size=len(movable))
    for j, a in (human_q_override or {}).items():          # tests only: e.g. an abducted arm
        hq[j] = a
    base_rpy = np.array([-np.pi / 2.0, 0, 0])
    return dict(draw._asdict(), hm=hm, hq=hm.clamp(hq), base_pos=np.array(base_pos), base_rpy=base_rpy, base_quat=X.quat_from_rpy(base_rpy))


class BedBathingSawyerReset:
    def __init__(self, blob, settle='drop'):
        assert blob.task_kind == L.TASK_BED_BATHING
        self.blob, self.settle = blob, settle
        self.mount = blob.meta.get('mount', 'toc')
        self.arm, self.mobile, self.search = None, None, None
        if self.mount == 'mobile':                                  # the Stretch: no arm chain to solve (env.py:282-293)
            from .reset import MobilePlacement
            self.mobile = MobilePlacement(blob)
        else:
            self.search = BasePoseSearch(blob, toc_base=[-0.2, 0, 0.975], ee_rpy=[0, np.pi / 2.0, 0])      # toc_base_pos_offset (sawyer.py:37), toc_ee_orient_rpy (sawyer.py:43)
            self.arm = self.search.arm
        self.bed = BedSurface(blob)

    def _human(self, gender, limit_scale):
        return human_model(gender, limit_scale)

    def _bed_top(self, x, y):
        return self.bed.top(x, y)

    def sample(self, rng, state_row, env_seed=0, impairment='random', gender='random', info=None, human_q_override=None):
        """Fill one state record (float32 view of length state_words) in place, with the 'drop' stand-in for the settle."""
        pre = self.pre_settle(rng, impairment, gender, human_q_override)
        pre['base_pos'] = self.bed.drop(pre['hm'], pre['base_pos'], pre['base_quat'], pre['hq'])
        return self.post_settle(rng, state_row, pre, env_seed, info)

    def pre_settle(self, rng, impairment='random', gender='random', human_q_override=None):
        return pose_in_air(rng, self.blob, impairment, gender, human_q_override, [-0.15, 0.2, 0.95])

    def post_settle(self, rng, state_row, pre, env_seed=0, info=None, attempt=0):
        """everything after the settle (bed_bathing.py:133-171), from the resting pose in `pre`"""
        b = self.blob
        v = b.view(state_row)
        draw, hm, hq, base_pos, base_quat = draw_of(pre), pre['hm'], pre['hq'], pre['base_pos'], pre['base_quat']
        hpos, hquat = hm.fk(base_pos, base_quat, hq)
        write_human_frames(v, b.meta['human_bodies'], hpos, hquat, base_pos, base_quat)
        shoulder, elbow, wrist = hpos[5], hpos[7], hpos[9]                         # bed_bathing.py:139-141
        if attempt == 0:
            pre['target_ee_pos'] = np.array([-0.6, 0.2, 1]) + rng.uniform(-0.05, 0.05, size=3)    # bed_bathing.py:147
        target_ee_pos = pre['target_ee_pos']
        prng = placement_rng(rng, env_seed, attempt)
        if self.mount == 'mobile':
            rb_pos, rb_quat, q = self.mobile.draw(prng)
            ngoal, manip = 0, 0.0
            tp, tq = self.mobile.kin.tool_pose(rb_pos, rb_quat, q)
        else:
            rb_pos, rb_quat, q_arm, ngoal, manip = self.search.search(prng, target_ee_pos, [shoulder, elbow, wrist])
            q = self.search.arm_joints(q_arm)
            tp, tq = self.search.tool_pose(rb_pos, rb_quat, q_arm)
        open_gripper(b, q)                                                         # bed_bathing.py:156
        # human.setup_joints(use_static_joints=True) after the settle (bed_bathing.py:134): every link static unless the impairment is tremor
        write_joints(v, b, q, np.array([hq[j] for j in b.meta['human_dynamic_joints']]), draw, frozen_unless_agent(b, draw), rb_pos, rb_quat)
        free = v['free'][0]
        free[:] = 0
        free[0, :3], free[0, 3:7] = tool_com_pose(b, 0, tp, tq)
        g = 0 if draw.gender == 'male' else 1
        nt = b.task_i_n('NT', 4)[2 * g] + b.task_i_n('NT', 4)[2 * g + 1]
        write_env_tail(v, draw, env_seed, nt)                                      # total_target_count (bed_bathing.py:187)
        alive = np.zeros(L.BB['ALIVE_WORDS'], dtype=np.uint32)
        for t in range(nt):
            alive[t >> 5] |= np.uint32(1 << (t & 31))
        v['task'][0, L.BB['ALIVE']:L.BB['ALIVE'] + L.BB['ALIVE_WORDS']] = alive.view(np.int32)
        if info is not None:
            info.update(gender=draw.gender, impairment=draw.impairment, limit_scale=draw.limit_scale, strength=draw.strength, tremors=draw.tremors,
                        toc_goals=ngoal, toc_manipulability=manip, target_ee_pos=target_ee_pos, human_q=hq, human_base=(base_pos, base_quat))
        return state_row


def make_states(blob, n, seed=1001, impairment='random', settler=None, checker=None, **kw):
    """n independent post-reset states; env i uses RandomState(seed + i).  With a `settler` (a callable advancing bed_settle
    state records by the 100 simulation steps of bed_bathing.py:130-131, e.g. RagdollSettler) the human is settled as a rag
    doll, all environments in one batch; without one the rigid 'drop' stand-in is used.  checker(states) -> AGX_COLLIDE_* flags
    (DeviceCollisionChecker) turns on init_robot_pose's collision rejection (needs the settler path)."""
    rs = BedBathingSawyerReset(blob, settle='drop' if settler is None else 'ragdoll')
    st = blob.new_state(n)
    infos = [{} for _ in range(n)]
    rngs = [np.random.RandomState(seed + i) for i in range(n)]
    if settler is None:
        for i in range(n):
            rs.sample(rngs[i], st[i:i + 1], env_seed=seed + i, impairment=impairment, info=infos[i], **kw)
        return st, infos
    pres = [rs.pre_settle(rngs[i], impairment=impairment, **kw) for i in range(n)]
    rest_on_bed(settler, pres)

    def place(i, attempt=0):
        rs.post_settle(rngs[i], st[i:i + 1], pres[i], env_seed=seed + i, info=infos[i], attempt=attempt)
    for i in range(n):
        place(i)
    flag_collisions(st, checker, place, infos)
    return st, infos
