"""End-effector (Cartesian) actions for the batched environments.

The reference's teleop_example.py / igibson_drinking_example.py drive the arm in Cartesian space: read robot.get_pos_orient(end effector), call
robot.ik(...) on a target pose, send (target_joint_angles - current_joint_angles) * 10 as the action.  EndEffectorControl does that for every
environment of a vec env (assistive_gym_amd.vec_env) in ONE launch of libagx's agx_ee_ik per step (csrc/agx_ik.hip): the command goes in, the
joint-space action comes out on the device, the inner env steps with it.  It presents the vec-env surface rollout.collect, ppo.PPOTrainer and
ppo.evaluate read, so a policy can be trained on end-effector deltas (`python -m assistive_gym.learn --train --ee-actions`).

The IK is the damped-least-squares iteration of host/kin.py (RobotKin.ik) in float32, not Bullet's.  Robots on wheels (Stretch) are not served.
"""
import torch


class _BlobProxy:
    """the inner env's model blob with the robot's action width replaced by the command's (rollout.agent_slices, ppo.make_policies)"""

    def __init__(self, blob, act_dim_robot):
        self._blob, self.act_dim_robot = blob, act_dim_robot

    def __getattr__(self, name):
        return getattr(self._blob, name)


class EndEffectorControl:
    """Wraps a vec env: act_dim = 6 x arms (mode 'delta') or 7 x arms ('absolute'), followed by the human's action columns of a co-op env.

    'delta':    per arm (dx, dy, dz, rx, ry, rz), each clipped to [-1, 1], then scaled by pos_step metres / rot_step radians: a world translation and
                a world rotation vector applied to the end effector's current pose;
    'absolute': per arm a world position and a quaternion (x, y, z, w).
    pos_step = 0.01, rot_step = 0.05 and gain = 10 are the reference example's (0.01 m and 0.05 rad per key press, action = joint difference x 10);
    damping = 0.05 is RobotKin.ik's.  iters = 8 is a STARTING VALUE NOBODY HAS TUNED: the example asks Bullet for 200 iterations per call, a
    command of one step moves the target by a centimetre, and the damped iteration has not been compared with Bullet's.
    The action the IK asks for is scaled per arm to a largest magnitude of 1 (the env clips to [-1, 1]: the direction survives)."""

    def __init__(self, env, mode='delta', pos_step=0.01, rot_step=0.05, iters=8, damping=0.05, gain=10.0):
        if mode not in ('delta', 'absolute'):
            raise ValueError("mode must be 'delta' or 'absolute'")
        self.env, self.mode, self.iters, self.damping, self.gain = env, mode, int(iters), float(damping), float(gain)
        self.arms = env.stepper.ee_arms()
        if self.arms == 0:
            raise ValueError('end-effector control needs an arm chain on a fixed base: %s has none (a robot on wheels is out of scope)' % getattr(env, '_model_name', 'this model'))
        self.per_arm = 6 if mode == 'delta' else 7
        self.cmd_dim = self.per_arm * self.arms
        self.n_human = env.act_dim - env.blob.act_dim_robot                       # the human's columns of a co-op env, behind the robot's
        self.act_dim, self.obs_dim = self.cmd_dim + self.n_human, env.obs_dim
        self.n_envs, self.device, self.episode_len = env.n_envs, env.device, env.episode_len
        self.blob = _BlobProxy(env.blob, self.cmd_dim)
        self._scale = torch.tensor(([pos_step] * 3 + [rot_step] * 3) * self.arms, dtype=torch.float32, device=self.device)
        self._target = torch.zeros((self.n_envs, self.cmd_dim), dtype=torch.float32, device=self.device)
        self._action = torch.zeros((self.n_envs, env.act_dim), dtype=torch.float32, device=self.device)      # columns of no chain stay 0
        self._pose = torch.zeros((self.n_envs, self.arms, 7), dtype=torch.float32, device=self.device)

    # what the inner env owns
    obs = property(lambda self: self.env.obs)
    env_offset = property(lambda self: self.env.env_offset)

    def reset(self, *a, **kw):
        return self.env.reset(*a, **kw)

    def close(self):
        self.env.close()

    def ee_pose(self):
        """[n_envs, arms, 7] device tensor: world position and quaternion (x, y, z, w) of every end effector, now"""
        self.env.stepper.ee_pose(self._pose, self.env._stream())
        return self._pose

    def joint_action(self, cmd):
        """the inner env's action for a command (the IK launch alone): [n_envs, inner act_dim], valid until the next call"""
        assert cmd.is_cuda and cmd.dtype == torch.float32 and cmd.shape == (self.n_envs, self.act_dim)
        if self.n_human:
            self._action[:, self.env.act_dim - self.n_human:] = cmd[:, self.cmd_dim:]
        if self.mode == 'delta':
            torch.mul(cmd[:, :self.cmd_dim].clamp(-1.0, 1.0), self._scale, out=self._target)
        else:
            self._target.copy_(cmd[:, :self.cmd_dim])
        self.env.stepper.ee_ik(self._target, self.mode, self.iters, self.damping, self.gain, action=self._action, stream=self.env._stream())
        return self._action

    def step(self, cmd, obs_out=None):
        return self.env.step(self.joint_action(cmd), obs_out)
