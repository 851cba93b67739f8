"""`python -m assistive_gym.learn`: the reference's command line (assistive_gym/learn.py:187-225) on the batched stepper.

    python -m assistive_gym.learn --env FeedingJaco-v1 --train --train-timesteps 2000000 --save-dir ./trained_models/
    python -m assistive_gym.learn --env FeedingJaco-v1 --evaluate --eval-episodes 100 --load-policy-path ./trained_models/

--train runs assistive_gym_amd.ppo.PPOTrainer on --n-envs lock-stepped environments of one GPU, resumes from the newest checkpoint under
--load-policy-path (learn.py:44-56), prints the line of learn.py:86 per iteration and keeps the newest checkpoint only (learn.py:89-93);
--evaluate prints the statistics of learn.py:172-183.  Flags beyond the reference's: --n-envs, --reset (the vec env's reset mode),
--deterministic (evaluate with the mean action) and --ee-actions (the policy commands end-effector deltas, 6 per arm, turned into joint actions by
the device-side IK: assistive_gym_amd/ee_control.py; a checkpoint belongs to the action space it was trained in).  --algo sac and --render are not built and say so.
"""
import argparse
import os
import sys


def build_parser():
    parser = argparse.ArgumentParser(description='RL for Assistive Gym')
    parser.add_argument('--env', default='ScratchItchJaco-v1', help='Environment to train on (default: ScratchItchJaco-v1)')
    parser.add_argument('--algo', default='ppo', help='Reinforcement learning algorithm')
    parser.add_argument('--seed', type=int, default=1, help='Random seed (default: 1)')
    parser.add_argument('--train', action='store_true', default=False, help='Whether to train a new policy')
    parser.add_argument('--render', action='store_true', default=False, help='Whether to render a single rollout of a trained policy')
    parser.add_argument('--evaluate', action='store_true', default=False, help='Whether to evaluate a trained policy over n_episodes')
    parser.add_argument('--train-timesteps', type=int, default=1000000, help='Number of simulation timesteps to train a policy (default: 1000000)')
    parser.add_argument('--save-dir', default='./trained_models/', help='Directory to save trained policy in (default ./trained_models/)')
    parser.add_argument('--load-policy-path', default='./trained_models/',
                        help='Path name to saved policy checkpoint (NOTE: Use this to continue training an existing policy, or to evaluate a trained policy)')
    parser.add_argument('--render-episodes', type=int, default=1, help='Number of rendering episodes (default: 1)')
    parser.add_argument('--eval-episodes', type=int, default=100, help='Number of evaluation episodes (default: 100)')
    parser.add_argument('--colab', action='store_true', default=False, help='Whether rendering should generate an animated png rather than open a window')
    parser.add_argument('--verbose', action='store_true', default=False, help='Whether to output more verbose prints')
    parser.add_argument('--n-envs', type=int, default=4096, help='Lock-stepped environments on the GPU (default: 4096)')
    parser.add_argument('--reset', default='pool', choices=('pool', 'device', 'host'), help="The batched environment's reset mode (default: pool)")
    parser.add_argument('--deterministic', action='store_true', default=False, help='Evaluate with the mean action instead of a sample')
    parser.add_argument('--ee-actions', action='store_true', default=False, help='Act in end-effector space: 6 delta components per arm through the device-side IK (default: joint actions)')
    return parser


def make_vec_env(env_name, n_envs, seed=1001, reset='pool', device=0, ee_actions=False):
    """the batched environment behind a gym id of the reference ('FeedingJaco-v1', 'ScratchItchPR2Human-v1', ...); ee_actions: wrapped in
    ee_control.EndEffectorControl (end-effector delta actions)"""
    if ee_actions:
        from .ee_control import EndEffectorControl
        return EndEffectorControl(make_vec_env(env_name, n_envs, seed=seed, reset=reset, device=device))
    from . import vec_env
    from .envs import ENV_IDS
    name = env_name.split(':')[-1]
    if name not in ENV_IDS:
        raise KeyError('%s is not built (built: %s)' % (env_name, sorted(ENV_IDS)))
    scalar = ENV_IDS[name]
    stem = name.split('-')[0]
    coop = bool(scalar.coop)
    base = stem[:-len('Human')] if coop else stem
    cls = getattr(vec_env, stem + 'VecEnv', None) or getattr(vec_env, base + 'VecEnv', None)
    if cls is None:
        return vec_env.AssistiveVecEnv(n_envs, device=device, seed=seed, reset=reset, model=scalar.model, coop=coop)
    return cls(n_envs, device=device, seed=seed, reset=reset, coop=coop)


def train(env_name, algo, timesteps_total=1000000, save_dir='./trained_models/', load_policy_path='', coop=False, seed=0, n_envs=4096, reset='pool', cfg=None, out=sys.stdout, ee_actions=False):
    """learn.py:71-94.  Returns (checkpoint path, trainer)."""
    from . import ppo
    env = make_vec_env(env_name, n_envs, reset=reset, ee_actions=ee_actions)
    trainer = ppo.PPOTrainer(env, cfg or ppo.PPOConfig.batched(n_envs), seed=seed, env_name=env_name)
    checkpoint_path = ppo.latest_checkpoint(load_policy_path, algo, env_name)
    if checkpoint_path is not None:
        trainer.restore(checkpoint_path)
        print('Resumed from %s' % checkpoint_path, file=out)
    if os.path.abspath(load_policy_path or '') != os.path.abspath(save_dir):
        checkpoint_path = None                                                   # only checkpoints of the directory being written are replaced
    while trainer.timesteps_total < timesteps_total:
        result = trainer.train()
        print(f"Iteration: {result['training_iteration']}, total timesteps: {result['timesteps_total']}, total time: {result['time_total_s']:.1f}, FPS: {result['timesteps_total']/result['time_total_s']:.1f}, mean reward: {result['episode_reward_mean']:.1f}, min/max reward: {result['episode_reward_min']:.1f}/{result['episode_reward_max']:.1f}"
              + (f", rollout/learn: {result['time_rollout_s']:.2f}/{result['time_learn_s']:.2f} s"), file=out)
        out.flush()
        ppo.remove_checkpoint(checkpoint_path)
        checkpoint_path = trainer.save(ppo.checkpoint_dir(save_dir, algo, env_name))
    env.close()
    return checkpoint_path, trainer


def evaluate_policy(env_name, algo, policy_path, n_episodes=100, coop=False, seed=0, verbose=False, n_envs=4096, reset='pool', deterministic=False, out=sys.stdout, ee_actions=False):
    """learn.py:133-184"""
    from . import ppo
    n_envs = max(1, min(n_envs, n_episodes))
    env = make_vec_env(env_name, n_envs, seed=1001 + seed, reset=reset, ee_actions=ee_actions)
    trainer = ppo.PPOTrainer(env, ppo.PPOConfig.batched(n_envs), seed=seed, env_name=env_name)
    path = ppo.latest_checkpoint(policy_path, algo, env_name)
    if path is None:
        print('No checkpoint under %s: evaluating an untrained policy' % policy_path, file=out)
    else:
        trainer.restore(path)
    stats = ppo.evaluate(env, trainer.policies, n_episodes, seed=seed, deterministic=deterministic)
    env.close()
    if verbose:
        print('Episodes: %d (%d environments)' % (stats['episodes'], n_envs), file=out)
    print('\n', '-' * 50, '\n', file=out)
    print('Reward Mean:', stats['reward_mean'], file=out)
    print('Reward Std:', stats['reward_std'], file=out)
    print('Force Mean:', stats['force_mean'], file=out)
    print('Force Std:', stats['force_std'], file=out)
    print('Task Success Mean:', stats['task_success_mean'], file=out)
    print('Task Success Std:', stats['task_success_std'], file=out)
    out.flush()
    return stats


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.algo != 'ppo':
        sys.exit('--algo %s is not built: this package trains with PPO only (assistive_gym_amd/ppo.py)' % args.algo)
    if args.render:
        sys.exit('--render is not built: there is no renderer behind the batched stepper')
    coop = 'Human' in args.env
    checkpoint_path = None
    if args.train:
        checkpoint_path, _ = train(args.env, args.algo, timesteps_total=args.train_timesteps, save_dir=args.save_dir, load_policy_path=args.load_policy_path, coop=coop,
                                   seed=args.seed, n_envs=args.n_envs, reset=args.reset, ee_actions=args.ee_actions)
    if args.evaluate:
        evaluate_policy(args.env, args.algo, checkpoint_path if checkpoint_path is not None else args.load_policy_path, n_episodes=args.eval_episodes, coop=coop,
                        seed=args.seed, verbose=args.verbose, n_envs=args.n_envs, reset=args.reset, deterministic=args.deterministic, ee_actions=args.ee_actions)
    return 0


if __name__ == '__main__':
    sys.exit(main())
