"""What the six numpy samplers of this package share: the draws every reset starts with (build_assistive_env + Human.init), the cache of human
models, the writers of the record fields every task fills the same way, the batch loop with init_robot_pose's collision rejection, and the
helper that runs a batch through a Stepper on the device (the settlers, the collision checker).  A sampler keeps what is its own: its joint
presets, its targets, its task words."""
from collections import namedtuple

import numpy as np

from ..model import xform as X
from ..model.human import HumanModel

D = np.deg2rad
IDENTITY = np.array([0, 0, 0, 1.0])

HumanDraw = namedtuple('HumanDraw', 'plane_friction gender impairment limit_scale strength tremors')


def draw_human(rng, impairment, gender, n_tremor, tremor_deg):
    """build_assistive_env (env.py:114-134) and Human.init (human.py:72-102), in the reference's order.  tremor_deg / n_tremor: 20 degrees on the 4
    head joints where the head is what the human controls (feeding, drinking: human.py:89-90), 10 on every controllable joint otherwise (:91-92)"""
    plane_friction = rng.uniform(0.025, 0.5)                                   # env.py:120
    if gender not in ('male', 'female'):
        gender = rng.choice(['male', 'female'])                                # human.py:76-77
    if impairment == 'random':
        impairment = rng.choice(['none', 'limits', 'weakness', 'tremor'])      # human.py:80-81
    elif impairment == 'no_tremor':
        impairment = rng.choice(['none', 'limits', 'weakness'])
    limit_scale = 1.0 if impairment != 'limits' else rng.uniform(0.5, 1.0)     # human.py:85
    strength = 1.0 if impairment != 'weakness' else rng.uniform(0.25, 1.0)     # human.py:86
    tremors = np.zeros(n_tremor)
    if impairment == 'tremor':
        tremors = rng.uniform(D(-tremor_deg), D(tremor_deg), size=n_tremor)
    rng.uniform(0.4, 0.8)                                                      # skin colour, human_creation.py:63
    return HumanDraw(plane_friction, gender, impairment, limit_scale, strength, tremors)


def draw_of(pre):
    """the HumanDraw of a pre-settle dictionary (reset_bed.pose_in_air; tests build such dictionaries by hand, with the keys they need)"""
    return HumanDraw(*(pre.get(k) for k in HumanDraw._fields))


_HUMANS = {}


def human_model(gender, limit_scale, cloth=False):
    """HumanModel(gender, limit_scale) of the last few draws (cloth: with the collision shapes the garment sees, dressing)"""
    key = (gender, round(float(limit_scale), 9), cloth)
    if key not in _HUMANS:
        if len(_HUMANS) > 64:
            _HUMANS.clear()
        _HUMANS[key] = HumanModel(gender, limit_scale, cloth=True) if cloth else HumanModel(gender, limit_scale)
    return _HUMANS[key]


def seated_base(gender):
    return np.array([0, 0.03, 0.89 if gender == 'male' else 0.86])            # human.py:102


# ---- writers -----------------------------------------------------------------------------------------------------------------------------------
def write_human_frames(v, bodies, hpos, hquat, base_pos, base_quat):
    """v['human']: the frames of the human's bodies (link < 0: its base)"""
    for k, link in enumerate(bodies):
        v['human'][0, k, :3], v['human'][0, k, 3:] = (base_pos, base_quat) if link < 0 else (hpos[link], hquat[link])


def open_gripper(blob, q):
    """the joints no action drives at their open position, set instantly (feeding.py:144 and the same line of every task)"""
    for d in range(blob.nrobot):
        if blob.robot_i(d, 'ACT') < 0:
            q[d] = min(max(blob.robot_f(d, 'QT0'), blob.robot_f(d, 'LOWER')), blob.robot_f(d, 'UPPER'))
    return q


def write_joints(v, blob, q, hq_dyn, draw, frozen, base_pos, base_quat):
    """robot and human joints at rest with the motors holding them, the tremor words, the frozen mask, the robot's base"""
    nr = blob.nrobot
    v['q'][0, :nr], v['qd'][0], v['qt'][0, :nr] = q, 0, q
    v['q'][0, nr:], v['qt'][0, nr:] = hq_dyn, hq_dyn
    v['tremor'][0], v['tremor_target'][0] = draw.tremors, hq_dyn             # human.py:123 target_joint_angles
    v['frozen'][0] = frozen
    v['limit_scale'][0] = draw.limit_scale
    v['base'][0, :3], v['base'][0, 3:] = base_pos, base_quat


def frozen_unless_agent(blob, draw):
    """every human joint static (mass 0, human.py:104-110) unless the human trembles or is controllable"""
    return 0 if (draw.impairment == 'tremor' or blob.is_coop) else (((1 << blob.nhdof) - 1) << blob.nrobot)


def write_reactive_hold(v, blob, draw, gain, force):
    """the dynamic arm of a human that is no agent is held by a reactive PD (human.py:108,124-127); an agent's motors are re-set every step (env.py:130-131,222)"""
    agent = blob.is_coop or draw.impairment == 'tremor'
    v['human_kp'][0] = 0.0 if agent else gain
    v['human_maxf'][0] = 0.0 if agent else force * draw.strength


def tool_com_pose(blob, body, tp, tq):
    """the record holds COM frames: base frame (tp, tq) of free body `body` -> its COM frame (URDF base frame o REF^-1)"""
    ip, iq = X.invert(blob.free_f(body, 'REFPOS', 3), blob.free_f(body, 'REFQUAT', 4))
    return X.compose(tp, tq, ip, iq)


def write_env_tail(v, draw, env_seed, total):
    """the env words every task ends with; total: what task_success is measured against (food, targets, water; 1 = a threshold task)"""
    v['plane_friction'][0] = draw.plane_friction
    v['gender'][0] = 0 if draw.gender == 'male' else 1
    v['iteration'][0] = 0
    v['task_success'][0] = 0
    v['total_food'][0] = total
    v['rng'][0, 0] = (env_seed * 2654435761 + 12345) & 0x7FFFFFFF
    v['rng'][0, 1] = (env_seed ^ 0x5bd1e995) & 0x7FFFFFFF


# ---- batches -------------------------------------------------------------------------------------------------------------------------------------
def placement_rng(rng, env_seed, attempt):
    """the random stream of the robot's placement: the sampler's own stream on the first attempt, a stream of its own on the re-draws
    of init_robot_pose's rejection loop (env.py:281), so that nothing else of the episode changes"""
    return rng if attempt == 0 else np.random.RandomState((env_seed * 7919 + 104729 * attempt) & 0x7FFFFFFF)


def reject_collisions(states, flags_of, resample, max_iterations=3):
    """init_robot_pose's loop (env.py:281-308): states whose robot or tool touches the human / the furniture (or whose arm is folded into
    itself) are placed again, at most max_iterations placements in total; resample(i, attempt) rewrites states[i].  Returns the final
    flags (a state still colliding after the last attempt is kept, as in the reference)."""
    flags = flags_of(states)
    for attempt in range(1, max_iterations):
        bad = np.flatnonzero(flags)
        if not len(bad):
            break
        for i in bad:
            resample(int(i), attempt)
        flags[bad] = flags_of(states[bad])
    return flags


def flag_collisions(states, checker, resample, infos):
    """reject_collisions when there is a checker (states -> AGX_COLLIDE_* flags, DeviceCollisionChecker); the final flags go into the infos"""
    if checker is not None:
        for info, f in zip(infos, reject_collisions(states, checker, resample)):
            info['collision_flags'] = int(f)


def sample_batch(n, seed, draw, checker, infos, states):
    """env i is drawn from RandomState(seed + i): draw(i, rng, attempt) fills states[i]; a re-draw after a collision starts from the same seed"""
    for i in range(n):
        draw(i, np.random.RandomState(seed + i), 0)
    flag_collisions(states, checker, lambda i, attempt: draw(i, np.random.RandomState(seed + i), attempt), infos)


class DeviceBatch:
    """A Stepper of n_envs environments that batches of up to n_envs records are run through: the batch is padded with its row 0, set, handed
    to `run(stepper)`, and the first len(batch) rows of the state (and of the garments, where some were given) come back.  Fails loudly
    without a GPU (the product path has no CPU fallback)."""

    def __init__(self, blob, n_envs, device=0):
        from ..libagx import Stepper
        self.blob, self.n = blob, n_envs
        self.ctx = Stepper(blob, n_envs, device)

    def _padded(self, rows):
        buf = np.zeros((self.n,) + rows.shape[1:], dtype=np.float32)
        buf[:len(rows)], buf[len(rows):] = rows, rows[:1]
        return buf

    def load(self, states, cloth=None):
        assert len(states) <= self.n
        self.ctx.set_state(self._padded(states))
        if cloth is not None:
            self.ctx.set_cloth(self._padded(cloth))

    def settle(self, states, n_sim_steps, cloth=None):
        n = len(states)
        self.load(states, cloth)
        self.ctx.settle(n_sim_steps)
        self.ctx.synchronize()
        return self.ctx.get_state()[:n] if cloth is None else (self.ctx.get_state()[:n], self.ctx.get_cloth()[:n])
