"""`assistive_gym.learn` / `python -m assistive_gym.learn` (assistive_gym/learn.py): re-exported from assistive_gym_amd.learn"""
import sys

from assistive_gym_amd.learn import build_parser, evaluate_policy, main, make_vec_env, train  # noqa: F401

if __name__ == '__main__':
    sys.exit(main())
