"""numpy restatement of agx_policy_act's noise (include/agx.h): Philox4x32-10 (oracle/reset_oracle.py: philox4x32, the generator of the device-side
resets) with key = the 64-bit value seed + env_offset + i and counter (k >> 2, step, 1, 0); output words w0..w3; (wa, wb) = (w0, w1) if k & 2 == 0
else (w2, w3); u1 = ((wa >> 8) + 0.5) 2^-24, u2 = (wb >> 8) 2^-24, r = sqrt(-2 ln u1); eps = r cos(2 pi u2) for even k, r sin(2 pi u2) for odd k.  float64."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
from reset_oracle import philox4x32            # noqa: E402

MASK64 = (1 << 64) - 1


def policy_eps(seed, env_offset, n_envs, steps, act_dim):
    """eps[i, s, k] (float64) of env i, the s-th entry of `steps`, action component k"""
    steps = list(steps)
    out = np.zeros((n_envs, len(steps), act_dim))
    for i in range(n_envs):
        key = (int(seed) + int(env_offset) + i) & MASK64
        for s, step in enumerate(steps):
            for blk in range((act_dim + 3) // 4):
                w = philox4x32((blk, int(step) & 0xFFFFFFFF, 1, 0), (key & 0xFFFFFFFF, key >> 32))
                for k in range(4 * blk, min(4 * blk + 4, act_dim)):
                    wa, wb = (w[0], w[1]) if k & 2 == 0 else (w[2], w[3])
                    u1, u2 = ((wa >> 8) + 0.5) / 16777216.0, (wb >> 8) / 16777216.0
                    r = math.sqrt(-2.0 * math.log(u1))
                    out[i, s, k] = r * (math.cos(2.0 * math.pi * u2) if k % 2 == 0 else math.sin(2.0 * math.pi * u2))
    return out
