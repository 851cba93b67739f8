"""gym.Env surface of the reference for the built hot paths (FeedingJaco-v1, BedBathingSawyer-v1 and their co-op flavours).

Mirrors, by name and behaviour, what assistive_gym/learn.py and env_viewer.py touch
(SURVEY 8b): classes ``FeedingJacoEnv`` (assistive_gym/envs/feeding_envs.py:29-31) and ``BedBathingSawyerEnv``
(assistive_gym/envs/bed_bathing_envs.py:23-25) with
``reset() -> obs``, ``step(a) -> (obs, reward, done, info)`` (feeding.py:12-43), ``seed``
(env.py:78-80), ``set_seed``, ``disconnect``, ``render`` (no-op: rendering is out of scope),
``action_space`` / ``observation_space`` (+ ``_robot`` / ``_human`` variants, env.py:42-49),
``action_robot_len`` ..., and the ``info`` keys of feeding.py:36.

Each scalar env is slot 0 of its own 1-environment stepper handle; the batched form is
assistive_gym_amd.vec_env.FeedingJacoVecEnv.  Physics always runs in libagx on the GPU: there is no
CPU fallback, constructing the env without a GPU raises.
"""
import numpy as np

from .blob import ModelBlob
from .reset_recipes import SETTLE_STEPS, HostSampler, sample_on_device      # noqa: F401 (SETTLE_STEPS: the feeding row's, as this module always exported it)

try:                                     # gym is optional here (not installed in the build image)
    import gym
    from gym import spaces
    from gym.utils import seeding
    _Base = gym.Env
except Exception:                        # minimal stand-ins with the attributes the callers read
    gym = None

    class _Box:
        def __init__(self, low, high, dtype=np.float32):
            self.low, self.high, self.dtype = np.asarray(low, dtype=dtype), np.asarray(high, dtype=dtype), dtype
            self.shape = self.low.shape
            self._rng = np.random.RandomState()

        def seed(self, seed=None):
            self._rng = np.random.RandomState(seed)

        def sample(self):
            return self._rng.uniform(self.low, self.high).astype(self.dtype)

        def contains(self, x):
            x = np.asarray(x)
            return x.shape == self.shape and np.all(x >= self.low) and np.all(x <= self.high)

    class spaces:                        # noqa: N801
        Box = _Box

    class seeding:                       # noqa: N801
        @staticmethod
        def np_random(seed=None):
            if seed is None:
                seed = np.random.SeedSequence().entropy % (2 ** 31)
            return np.random.RandomState(int(seed) % (2 ** 32)), seed

    class _Base:
        metadata = {}


def _box(n, bound):
    v = np.ones(n, dtype=np.float32) * bound
    return spaces.Box(low=-v, high=v, dtype=np.float32)


class _Agent:
    """The attributes of the reference's Robot / Human / Tool objects that learn.py, env_viewer.py and user scripts read
    (controllable_joint_indices, agent.py:21; Robot tables, robot.py:6-39).  Of the physics calls on them, get_closest_points is built (env.robot,
    env.tool and env.human of a scalar env) and the robot's end-effector calls, _Robot below; get_contact_points and link frames are not."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def get_closest_points(self, agentB, distance=4.0, linkA=None, linkB=None):
        """agent.py:118-130: (linkA, linkB, posA, posB, distance) lists, one entry per pair of a collider of this agent and a collider of
        `agentB` (optionally of links linkA / linkB only) whose surfaces are closer than `distance`, in pair order; a negative distance is a
        penetration.  Bullet reports per collision shape of its own bodies; this reports per collider of the model blob (spheres, capsules
        and convex hulls with a margin: what the stepper collides), one closest point per collider pair, answered by the batched query of
        assistive_gym_amd/proximity.py on the env's one environment."""
        from .proximity import ProximityQuery
        env, tag_a, tag_b = getattr(self, '_env', None), getattr(self, '_tag', None), getattr(agentB, '_tag', None)
        if env is None or tag_a is None or tag_b is None:
            raise NotImplementedError('get_closest_points: only between env.robot, env.tool and env.human')
        key = (tag_a, tag_b, float(distance), linkA, linkB)
        cache = env.__dict__.setdefault('_proximity_queries', {})
        st = env._ensure_stepper()
        if key not in cache or cache[key].stepper is not st:
            cache[key] = ProximityQuery(st, [((tag_a, [linkA]) if linkA is not None else tag_a, (tag_b, [linkB]) if linkB is not None else tag_b)], distance)
        q = cache[key]
        out = q.closest()
        st.synchronize()
        kind = out['kind'][0].cpu().numpy()
        dist, pa, pb = (out[k][0].cpu().numpy().astype(np.float64) for k in ('distance', 'point_a', 'point_b'))
        link = [q.blob.collider(int(c))['link'] for c in range(q.blob.h['NCOLL'])]
        hit = [k for k in range(len(q.pairs)) if kind[k] != 0]
        return ([link[q.pairs[k, 0]] for k in hit], [link[q.pairs[k, 1]] for k in hit], [tuple(pa[k]) for k in hit], [tuple(pb[k]) for k in hit],
                [float(dist[k]) for k in hit])


class _EndEffector(int):
    """A handle robot.get_pos_orient / robot.ik accept: the reference's link number of the end effector (an int, as robot.right_end_effector
    is there) that also says which arm chain of the stepper it names.  -1 where the robot tables (model/compiler.py) do not carry the number:
    a sentinel only these two calls take."""

    def __new__(cls, link, arm):
        self = super().__new__(cls, link)
        self.arm = arm
        return self


class _Robot(_Agent):
    """The robot of a scalar env: the attribute bag plus the end-effector calls of the reference's teleoperation loop (teleop_example.py:
    robot.get_pos_orient(robot.right_end_effector), robot.get_joint_angles(robot.right_arm_joint_indices), robot.ik(...)), answered by the
    stepper's agx_ee_pose / agx_ee_ik for the env's one environment.  The IK is the damped-least-squares iteration of host/kin.py in float32 on
    the device, not Bullet's; the frame of a link other than an end effector and contacts are not built."""

    def _bind(self, env, base):
        from .model import compiler as L
        self._env, self._base = env, base
        x0 = base.h['OFF_RESET']
        two = base.has_reset_generator and bool(int(base.i[x0 + L.X_['FLAGS']]) & 512)
        chains = [[int(d) for d in base.i[x0 + L.X_[k]:x0 + L.X_[k] + 7]] for k in (['CHAIN', 'CHAIN2'] if two else ['CHAIN'])] if base.has_reset_generator else []
        name = base.meta.get('robot')
        for arm, chain in enumerate(chains):
            if any(d < 0 or d >= base.nrobot for d in chain) or len(set(chain)) != 7:
                continue                                           # a robot on wheels: its chain words are unused
            pb = [base.robot_i(d, 'PB_INDEX') for d in chain]
            # the reference's link number and the side of this arm, where a robot table lists these joints (the right arms of PR2 / Baxter have a
            # table of their own; a single-arm robot answers to both sides, as its right_* and left_* lists are the same in the reference)
            tables = [('right', L.ROBOT_RIGHT.get(name)), ('left' if name in L.ROBOT_RIGHT else 'both', L.ROBOT_BASE.get(name)), ('both', L.FEEDING_ROBOTS.get(name))]
            side, link = next(((sd, t['ee_pb']) for sd, t in tables if t and list(t.get('arm', ())) == pb), ('left' if arm else ('right' if two else 'both'), -1))
            for sd in (('right', 'left') if side == 'both' else (side,)):
                setattr(self, sd + '_end_effector', _EndEffector(link, arm))
                setattr(self, sd + '_arm_joint_indices', list(pb))
                setattr(self, sd + '_arm_ik_indices', list(range(7)))       # robot.ik returns the arm's seven angles: the indices into Bullet's solution vector have no meaning here
        self._chains = chains

    def _arm(self, link):
        if not isinstance(link, _EndEffector):
            raise NotImplementedError('only the end effector is built: pass robot.right_end_effector / robot.left_end_effector (link frames and contacts of other links are not)')
        return link.arm

    def _poses(self):
        import torch
        st = self._env._ensure_stepper()
        out = torch.zeros((1, max(1, st.ee_arms()), 7), dtype=torch.float32, device='cuda:%d' % self._env.device)
        st.ee_pose(out)                                            # raises for a robot on wheels (agx_ee_arms is 0)
        st.synchronize()
        return out

    def get_pos_orient(self, link, center_of_mass=False, convert_to_realworld=False):
        """agent.py:130-140 for the end effector: (world position [3], quaternion x y z w [4]) of its link frame"""
        if center_of_mass or convert_to_realworld:
            raise NotImplementedError('get_pos_orient: only the link frame in world coordinates is built')
        pose = self._poses()[0, self._arm(link)].cpu().numpy().astype(np.float64)
        return pose[:3], pose[3:]

    def get_joint_angles(self, indices=None):
        """agent.py:84-90: angles of the joints with these PyBullet indices (default: the controllable ones)"""
        base = self._base
        dof = {base.robot_i(d, 'PB_INDEX'): d for d in range(base.nrobot)}
        q = base.view(self._env._ensure_stepper().get_state())['q'][0]
        return np.array([q[dof[j]] for j in (self.controllable_joint_indices if indices is None else indices)], dtype=np.float64)

    def ik(self, target_joint, target_pos, target_orient=None, ik_indices=None, max_iterations=200, use_current_as_rest=False, **ignored):
        """agent.py:252-274: target joint angles of the arm that carries `target_joint` for a world pose; target_orient None keeps the current
        orientation.  Up to max_iterations (at most 1000) damped-least-squares iterations from the current angles, stopping at 1e-4; limits are the
        joint limits (Bullet's rest poses, joint ranges and its null-space term are not reproduced)."""
        import torch
        arm = self._arm(target_joint)
        st = self._env._ensure_stepper()
        target = self._poses().clone()                             # the other arm of a two-armed robot aims at where it is
        target[0, arm, :3] = torch.as_tensor(np.asarray(target_pos, dtype=np.float32))
        if target_orient is not None:
            target[0, arm, 3:] = torch.as_tensor(np.asarray(target_orient, dtype=np.float32))
        q_out = torch.zeros_like(target)
        st.ee_ik(target.reshape(1, -1), 'absolute', iters=max(1, min(int(max_iterations), 1000)), q_out=q_out)
        st.synchronize()
        return q_out[0, arm].cpu().numpy().astype(np.float64)


class AssistiveEnv(_Base):
    """Common part of the scalar envs (AssistiveEnv, assistive_gym/envs/env.py:21-67)."""
    coop = False
    model = None            # blob name
    task = None

    def __init__(self, device=0):
        self.time_step, self.frame_skip = 0.02, 5                                    # env.py:21
        base = ModelBlob.load(self.model)
        self.blob = base.coop() if self.coop else base
        self.device = device
        self.action_robot_len, self.obs_robot_len = base.act_dim, base.obs_dim       # env.py:40-44, feeding.py:10
        self.action_human_len = self.blob.act_dim - base.act_dim                     # controllable human joints (feeding_envs.py:11)
        self.obs_human_len = self.blob.obs_dim - base.obs_dim                        # feeding.py:10: 23 in co-op
        self.action_space = _box(self.action_robot_len + self.action_human_len, 1.0)               # env.py:42
        self.observation_space = _box(self.obs_robot_len + self.obs_human_len, 1000000000.0)       # env.py:45
        self.action_space_robot, self.observation_space_robot = _box(self.action_robot_len, 1.0), _box(self.obs_robot_len, 1000000000.0)
        self.action_space_human, self.observation_space_human = _box(self.action_human_len, 1.0), _box(self.obs_human_len, 1000000000.0)
        self.gui = False
        self.iteration = 0
        self.task_success = 0
        self.total_force_on_human = 0.0
        self._stepper, self._host_sampler = None, None
        arm_pb = [base.robot_i(d, 'PB_INDEX') for d in sorted((d for d in range(base.nrobot) if base.robot_i(d, 'ACT') >= 0 and base.robot_i(d, 'ACT_SRC') == 0), key=lambda d: base.robot_i(d, 'ACT'))]
        if base.act_dim_robot == 2 * len(arm_pb):                                     # a single-arm robot with robot_arm = 'both' (robot.py:16)
            arm_pb = arm_pb + arm_pb
        hum_pb = [self.blob.robot_i(d, 'PB_INDEX') for d in range(base.nrobot, base.ndof)] if self.coop else []
        mobile = base.h['BASE_LINK'] > 0                                              # robot.py:11: 'wheel' in controllable_joints
        d0 = next(d for d in range(base.nrobot) if base.robot_i(d, 'ACT') >= 0)
        self.robot = _Robot(controllable_joint_indices=arm_pb, mobile=mobile, motor_gains=base.robot_f(d0, 'KP'), motor_forces=base.robot_f(d0, 'MAXF'),
                            wheel_joint_indices=[base.robot_i(d, 'PB_INDEX') for d in range(base.nrobot) if base.robot_i(d, 'OBS_SKIP') and base.robot_i(d, 'ACT_SRC') == 0 and base.robot_i(d, 'ACT') >= 0])
        self.robot._bind(self, base)
        self.human = _Agent(controllable_joint_indices=hum_pb, controllable=self.coop)
        self.tool = _Agent()
        for agent, tag in ((self.robot, 'robot'), (self.tool, 'tool'), (self.human, 'human')):      # what get_closest_points asks about
            agent._env, agent._tag = self, tag
        self.camera_width, self.camera_height, self.view_matrix, self.projection_matrix = None, None, None, None
        self.seed(1001)                                                               # env.py:21,30

    # ---- gym API ------------------------------------------------------------------------------
    def seed(self, seed=None):
        self.np_random, seed = seeding.np_random(seed)
        return [seed]

    def set_seed(self, seed=1000):
        self.np_random.seed(seed)

    def _ensure_stepper(self):
        if self._stepper is None:
            from .libagx import Stepper          # raises without the HIP library / a GPU
            self._stepper = Stepper(self.blob, 1, self.device)
        return self._stepper

    def _draw_seed(self):
        """62 bits from the gym-seeded generator: the key of the device-side reset generator's counter RNG"""
        r = self.np_random
        draw = r.integers if hasattr(r, 'integers') else r.randint
        return (int(draw(0, 2 ** 31 - 1)) << 31) | int(draw(0, 2 ** 31 - 1))

    sampler = 'host'          # where reset() is sampled: 'device' (the reset generator, csrc/agx_reset.h) or 'host' (the numpy sampler under host/)

    def reset(self):
        """<Task>Env.reset by the task's recipe (reset_recipes.py), as vec_env.build_reset_pool builds one pool entry.  'device': sampled by
        the reset generator (human, IK restarts with collision rejection, tool, targets), then the recipe's settle steps.  'host': the draws,
        the base pose search and the IK restated in numpy (host/) around the settles of the recipe, which run on the device (the rag doll on
        the bed_settle model, the arm's fall, the garment's 50 steps), with the device's collision pass rejecting colliding placements; the
        result is injected into the stepper."""
        st = self._ensure_stepper()
        self.reset_seed = self._draw_seed()
        if self.sampler == 'device':
            sample_on_device(st, self.blob, self.reset_seed, 'random', fused=False)
        else:
            if self._host_sampler is None:
                self._host_sampler = HostSampler(self.blob, 1, self.device)
            self._host_sampler.inject(st, *self._host_sampler(1, self.reset_seed % (2 ** 31)))
        self.iteration, self.task_success = 0, 0
        return self._split_obs(st.observe_host()[0].astype(np.float64))

    def _split_obs(self, obs):
        if not self.coop:
            return obs
        return {'robot': obs[:self.obs_robot_len], 'human': obs[self.obs_robot_len:]}              # feeding.py:110-111

    def step(self, action):
        if self.coop and isinstance(action, dict):                                                 # feeding.py:13-14
            action = np.concatenate([action['robot'], action['human']])
        action = np.asarray(action, dtype=np.float32)
        n_act = self.action_robot_len + self.action_human_len
        if action.shape != (n_act,):
            # the reference prints and exit()s (env.py:198-200); a library must not kill the process
            raise ValueError('Received agent actions of length %d does not match expected action length of %d' % (action.size, n_act))
        obs, rew, done, info = self._ensure_stepper().step_host(action[None])
        self.iteration += 1
        self.total_force_on_human = float(info[0, 0])
        out_info = {'total_force_on_human': float(info[0, 0]), 'task_success': int(info[0, 1]),
                    'action_robot_len': self.action_robot_len, 'action_human_len': self.action_human_len,
                    'obs_robot_len': self.obs_robot_len, 'obs_human_len': self.obs_human_len}      # feeding.py:36
        o, r, d = self._split_obs(obs[0].astype(np.float64)), float(rew[0]), bool(done[0])
        if not self.coop:
            return o, r, d, out_info
        # co-optimisation: per-agent dictionaries (feeding.py:41-43)
        return o, {'robot': r, 'human': r}, {'robot': d, 'human': d, '__all__': d}, {'robot': out_info, 'human': out_info}

    def render(self, mode='human'):
        return None          # GUI / EGL rendering is outside the hot path

    def setup_camera(self, camera_eye=(0.5, -0.75, 1.5), camera_target=(-0.2, 0, 0.75), fov=60, camera_width=1920 // 4, camera_height=1080 // 4, garment=False):
        """env.py:342-346.  The camera is the batched one (assistive_gym_amd/camera.py) on this environment's stepper: it draws the collision geometry
        and, with garment=True in a Dressing* environment, the gown"""
        self.camera_width, self.camera_height, self._camera_garment = camera_width, camera_height, bool(garment)
        self.view_matrix, self.projection_matrix = ('eye', tuple(camera_eye), tuple(camera_target)), fov
        self._camera = None

    def setup_camera_rpy(self, camera_target=(-0.2, 0, 0.75), distance=1.5, rpy=(0, -35, 40), fov=60, camera_width=1920 // 4, camera_height=1080 // 4, garment=False):
        """env.py:348-352: rpy = (roll, pitch, yaw) in degrees, the z axis up; garment as in setup_camera"""
        self.camera_width, self.camera_height, self._camera_garment = camera_width, camera_height, bool(garment)
        self.view_matrix, self.projection_matrix = ('rpy', tuple(camera_target), distance, tuple(rpy)), fov
        self._camera = None

    def get_camera_image_depth(self, light_pos=(0, -3, 1), shadow=False, ambient=0.8, diffuse=0.3, specular=0.1):
        """env.py:354-359 -> (image uint8 [h, w, 4], depth buffer float32 [h, w] in Bullet's convention: 0 at the near plane, 1 at the far plane and
        where nothing is hit).  `shadow` and `specular` are accepted and ignored: the camera casts no shadows and has no specular term."""
        assert self.view_matrix is not None, 'You must call env.setup_camera() or env.setup_camera_rpy() before getting a camera image'   # env.py:355
        from .camera import BatchedCamera, bullet_depth
        if getattr(self, '_camera', None) is None or self._camera.stepper is not self._ensure_stepper():
            self._camera = BatchedCamera(self._ensure_stepper(), self.camera_width, self.camera_height, fov=self.projection_matrix)
            if self.view_matrix[0] == 'rpy':
                self._camera.setup_rpy(self.view_matrix[1], self.view_matrix[2], self.view_matrix[3], self.projection_matrix)
            else:
                self._camera.setup(self.view_matrix[1], self.view_matrix[2], self.projection_matrix)
            self._camera.set_garment(getattr(self, '_camera_garment', False))
        out = self._camera.render(light_pos=light_pos, ambient=ambient, diffuse=diffuse)
        return out['rgba'][0].cpu().numpy(), bullet_depth(out['depth'][0].cpu().numpy().astype(np.float64)).astype(np.float32)

    def get_euler(self, quaternion):
        """env.py:342-343 (p.getEulerFromQuaternion): fixed-axis roll, pitch, yaw of a quaternion (x, y, z, w)"""
        x, y, z, w = np.asarray(quaternion, dtype=np.float64) / np.linalg.norm(quaternion)
        return np.array([np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), np.arcsin(np.clip(2 * (w * y - z * x), -1.0, 1.0)),
                         np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))])

    def get_quaternion(self, euler):
        """env.py:345-346 (p.getQuaternionFromEuler); a quaternion (4 values) is passed through"""
        from .model import xform
        euler = np.asarray(euler, dtype=np.float64)
        return euler if len(euler) == 4 else xform.quat_from_rpy(euler)

    def disconnect(self):
        if self._stepper is not None:
            self._stepper.close()
            self._stepper = None

    close = disconnect

    # ---- state injection (no reference equivalent; parity protocol of SURVEY 8c) ----------------
    def get_state(self):
        return self._ensure_stepper().get_state()[0]

    def set_state(self, state):
        self._ensure_stepper().set_state(np.asarray(state, dtype=np.float32).reshape(1, -1))


class FeedingJacoEnv(AssistiveEnv):
    """FeedingJaco-v1: Jaco arm on a wheelchair feeds a static (non-cooperating) human."""
    model, task, sampler = 'feeding_jaco', 'feeding', 'device'


class FeedingJacoHumanEnv(FeedingJacoEnv):
    """FeedingJacoHuman-v1 (feeding_envs.py:64-67): the human's head joints are controllable; actions,
    observations, rewards, dones and infos are per-agent dictionaries as RLlib's MultiAgentEnv expects."""
    coop = True


class FeedingSawyerEnv(FeedingJacoEnv):
    """FeedingSawyer-v1 (feeding_envs.py:25-27): a free-standing robot; its base pose comes from the base pose search on the host
    (host/reset.py + host/reset_bed.py) with the device's collision pass rejecting colliding placements, then the 25 settle steps."""
    model, sampler = 'feeding_sawyer', 'host'


class FeedingSawyerHumanEnv(FeedingSawyerEnv):
    """FeedingSawyerHuman-v1 (feeding_envs.py:51-54)"""
    coop = True


class FeedingBaxterEnv(FeedingSawyerEnv):
    """FeedingBaxter-v1 (feeding_envs.py:21-23): Baxter's right arm"""
    model = 'feeding_baxter'


class FeedingBaxterHumanEnv(FeedingBaxterEnv):
    """FeedingBaxterHuman-v1 (feeding_envs.py:46-49)"""
    coop = True


class FeedingPandaEnv(FeedingJacoEnv):
    """FeedingPanda-v1 (feeding_envs.py:35-37): the same task with the wheelchair-mounted Franka Panda (agents/panda.py)."""
    model = 'feeding_panda'


class FeedingPandaHumanEnv(FeedingPandaEnv):
    """FeedingPandaHuman-v1 (feeding_envs.py:69-73)"""
    coop = True


class _PairState:
    """the garment / the water lives outside the state record: a state is the pair (record, array[2][nodes][3])"""

    def get_state(self):
        st = self._ensure_stepper()
        return st.get_state()[0], st.get_cloth()[0]

    def set_state(self, state):
        if not (isinstance(state, (tuple, list)) and len(state) == 2):
            raise ValueError('a %s state is the pair (state record, %s): pass what get_state() returned' % (self.task, 'water' if self.task == 'drinking' else 'garment'))
        st = self._ensure_stepper()
        st.set_state(np.asarray(state[0], dtype=np.float32).reshape(1, -1))
        st.set_cloth(np.ascontiguousarray(state[1], dtype=np.float32)[None])


class DrinkingJacoEnv(_PairState, AssistiveEnv):
    """DrinkingJaco-v1 (drinking_envs.py:29-31): the wheelchair-mounted Jaco tilts a cup with 64 water particles at the person's mouth.
    The water lives next to the state record on the device (float32 [2, 64, 3]: positions, velocities)."""
    model, task, sampler = 'drinking_jaco', 'drinking', 'device'


class DrinkingJacoHumanEnv(DrinkingJacoEnv):
    """DrinkingJacoHuman-v1 (drinking_envs.py:56-59): the human's head joints are controllable too"""
    coop = True


class BedBathingSawyerEnv(AssistiveEnv):
    """BedBathingSawyer-v1 (bed_bathing_envs.py:23-25): Sawyer wipes the right arm of a human lying on a bed."""
    model, task = 'bed_bathing_sawyer', 'bed_bathing'


class BedBathingSawyerHumanEnv(BedBathingSawyerEnv):
    """BedBathingSawyerHuman-v1 (bed_bathing_envs.py:57-61): the human's right arm (10 joints) is controllable; the pose-dependent
    arm limits (human.py:134-152, the Keras classifier) run after every substep; per-agent dictionaries as in the reference."""
    coop = True


class ScratchItchPR2Env(AssistiveEnv):
    """ScratchItchPR2-v1 (scratch_itch_envs.py:17-19): the PR2's left arm scratches a target on the seated human's right arm."""
    model, task = 'scratch_itch_pr2', 'scratch_itch'


class ScratchItchPR2HumanEnv(ScratchItchPR2Env):
    """ScratchItchPR2Human-v1 (scratch_itch_envs.py:41-44; BASELINE config 4): the human's right arm (10 joints) is controllable,
    the pose-dependent arm limits run after every substep; actions {'robot': a[7], 'human': a[10]}, observations 30 + 34."""
    coop = True


class ScratchItchJacoEnv(ScratchItchPR2Env):
    """ScratchItchJaco-v1 (scratch_itch_envs.py:29-31; the default environment of the reference's env_viewer.py / learn.py): the
    wheelchair-mounted Jaco holds the scratcher.  reset() is sampled on the device (agx_sample_reset: human, IK with random restarts and
    collision rejection, tool, target on the arm), as FeedingJacoEnv's."""
    model, sampler = 'scratch_itch_jaco', 'device'


class ScratchItchJacoHumanEnv(ScratchItchJacoEnv):
    coop = True


class ScratchItchPandaEnv(ScratchItchJacoEnv):
    """ScratchItchPanda-v1 (scratch_itch_envs.py:37-39): as ScratchItchJaco, with the wheelchair-mounted Panda"""
    model = 'scratch_itch_panda'


class ScratchItchPandaHumanEnv(ScratchItchPandaEnv):
    coop = True


class ScratchItchSawyerEnv(ScratchItchPR2Env):
    """ScratchItchSawyer-v1 (scratch_itch_envs.py:25-27)"""
    model = 'scratch_itch_sawyer'


class ScratchItchSawyerHumanEnv(ScratchItchSawyerEnv):
    coop = True


class DressingBaxterEnv(_PairState, AssistiveEnv):
    """DressingBaxter-v1 (dressing_envs.py:19-21; BASELINE config 5): Baxter's left arm pulls the sleeve of a hospital gown over the left
    arm of the seated human.  The garment (3,966 nodes) lives next to the state record on the device."""
    model, task = 'dressing_baxter', 'dressing'


class DressingBaxterHumanEnv(DressingBaxterEnv):
    """DressingBaxterHuman-v1 (dressing_envs.py:51-55): the human's left arm (10 joints) is controllable, the pose-dependent arm limits
    run after every stepSimulation; actions {'robot': a[7], 'human': a[10]}, observations 24 + 28."""
    coop = True


class ArmManipulationSawyerEnv(AssistiveEnv):
    """ArmManipulationSawyer-v1 (arm_manipulation_envs.py:23-25): Sawyer lifts the limp right arm of a human lying on a bed back onto
    the body with a scooper.  robot_arm = 'both' on a single-arm robot: 14 actions (the arm joints twice, robot.py:16)."""
    model, task = 'arm_manipulation_sawyer', 'arm_manipulation'


class ArmManipulationSawyerHumanEnv(ArmManipulationSawyerEnv):
    """ArmManipulationSawyerHuman-v1 (arm_manipulation_envs.py:57-61): the human's right arm (10 joints) is controllable;
    actions {'robot': a[14], 'human': a[10]}, observations 45 + 42."""
    coop = True


ENV_IDS = {'FeedingSawyer-v1': FeedingSawyerEnv, 'FeedingSawyerHuman-v1': FeedingSawyerHumanEnv, 'FeedingBaxter-v1': FeedingBaxterEnv, 'FeedingBaxterHuman-v1': FeedingBaxterHumanEnv,
           'ScratchItchJaco-v1': ScratchItchJacoEnv, 'ScratchItchJacoHuman-v1': ScratchItchJacoHumanEnv, 'ScratchItchPanda-v1': ScratchItchPandaEnv,
           'ScratchItchPandaHuman-v1': ScratchItchPandaHumanEnv, 'ScratchItchSawyer-v1': ScratchItchSawyerEnv, 'ScratchItchSawyerHuman-v1': ScratchItchSawyerHumanEnv,
           'FeedingPanda-v1': FeedingPandaEnv, 'FeedingPandaHuman-v1': FeedingPandaHumanEnv, 'ArmManipulationSawyer-v1': ArmManipulationSawyerEnv, 'ArmManipulationSawyerHuman-v1': ArmManipulationSawyerHumanEnv, 'DressingBaxter-v1': DressingBaxterEnv, 'DressingBaxterHuman-v1': DressingBaxterHumanEnv, 'ScratchItchPR2-v1': ScratchItchPR2Env, 'ScratchItchPR2Human-v1': ScratchItchPR2HumanEnv, 'FeedingJaco-v1': FeedingJacoEnv, 'FeedingJacoHuman-v1': FeedingJacoHumanEnv, 'BedBathingSawyer-v1': BedBathingSawyerEnv,
           'BedBathingSawyerHuman-v1': BedBathingSawyerHumanEnv, 'DrinkingJaco-v1': DrinkingJacoEnv, 'DrinkingJacoHuman-v1': DrinkingJacoHumanEnv}

# ---- further robots of a task: the same env code with another model blob (model/compiler.py ROBOT_BASE / ROBOT_TASK) -----------------------
def _robot_flavours(base_cls, task_name, robots, ref):
    for robot, model in robots:
        cls = type('%s%sEnv' % (task_name, robot), (base_cls,), {'model': model, '__doc__': '%s%s-v1 (%s): %s with the %s' % (task_name, robot, ref, base_cls.__name__, robot)})
        coop_cls = type('%s%sHumanEnv' % (task_name, robot), (cls,), {'coop': True, '__doc__': '%s%sHuman-v1 (%s): the human is controllable too' % (task_name, robot, ref)})
        globals()[cls.__name__], globals()[coop_cls.__name__] = cls, coop_cls
        ENV_IDS['%s%s-v1' % (task_name, robot)] = cls
        ENV_IDS['%s%sHuman-v1' % (task_name, robot)] = coop_cls


_robot_flavours(BedBathingSawyerEnv, 'BedBathing', [('Jaco', 'bed_bathing_jaco'), ('Panda', 'bed_bathing_panda'), ('PR2', 'bed_bathing_pr2'), ('Baxter', 'bed_bathing_baxter'), ('Stretch', 'bed_bathing_stretch')],
                'bed_bathing_envs.py:15-37,45-79')
_robot_flavours(FeedingSawyerEnv, 'Feeding', [('PR2', 'feeding_pr2'), ('Stretch', 'feeding_stretch')], 'feeding_envs.py:17-19,33-35,41-44,60-63')
_robot_flavours(DressingBaxterEnv, 'Dressing', [('Sawyer', 'dressing_sawyer'), ('Jaco', 'dressing_jaco'), ('Panda', 'dressing_panda'), ('PR2', 'dressing_pr2'), ('Stretch', 'dressing_stretch')], 'dressing_envs.py:23-37,56-79')
_robot_flavours(ArmManipulationSawyerEnv, 'ArmManipulation', [('Jaco', 'arm_manipulation_jaco'), ('Panda', 'arm_manipulation_panda'), ('PR2', 'arm_manipulation_pr2'),
                                                              ('Baxter', 'arm_manipulation_baxter')], 'arm_manipulation_envs.py:15-37,41-79')
_robot_flavours(ScratchItchPR2Env, 'ScratchItch', [('Baxter', 'scratch_itch_baxter'), ('Stretch', 'scratch_itch_stretch')], 'scratch_itch_envs.py:21-23,31-33,46-50,58-62')
_robot_flavours(DrinkingJacoEnv, 'Drinking', [('PR2', 'drinking_pr2'), ('Baxter', 'drinking_baxter'), ('Sawyer', 'drinking_sawyer'), ('Stretch', 'drinking_stretch'), ('Panda', 'drinking_panda')],
                'drinking_envs.py:15-27,33-55,61-67')


def make(env_id):
    """`gym.make('assistive_gym:FeedingJaco-v1')` equivalent, with the TimeLimit of 200 steps folded
    into the env itself (done = iteration >= 200, feeding.py:37; assistive_gym/__init__.py:11)."""
    name = env_id.split(':')[-1]
    if name not in ENV_IDS:
        raise KeyError('%s is not built yet (hot-path scope: %s)' % (env_id, sorted(ENV_IDS)))
    return ENV_IDS[name]()


if gym is not None:       # same ids the reference registers (assistive_gym/__init__.py:6-12)
    try:
        from gym.envs.registration import register
        register(id='FeedingJaco-v1', entry_point='assistive_gym_amd.envs:FeedingJacoEnv', max_episode_steps=200)
        register(id='BedBathingSawyer-v1', entry_point='assistive_gym_amd.envs:BedBathingSawyerEnv', max_episode_steps=200)
        register(id='ScratchItchPR2-v1', entry_point='assistive_gym_amd.envs:ScratchItchPR2Env', max_episode_steps=200)
    except Exception:
        pass
