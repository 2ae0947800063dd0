"""The device parameter-space noise (struct smx_param_noise, include/surreal_amd.h) restated in numpy float64 from its
definition, on the Philox restatement of noise_ref.py / philox_ref.py.  Tests only.

    z(seed, g, q, i) = component i & 3 of the block at counter (g, q, i >> 2, 0x504E0001), key = the seed's two words,
                       through the exploration stream's word -> normal conversion (two Box-Muller pairs a block)
    perturbed_i      = w_i + sigma * z          over the actor's flat parameters W1 | b1 | W2 | b2 | W3 | b3
"""
import numpy as np

import noise_ref as NR
from philox_ref import MASK

TAG = 0x504E0001
ORDER = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')


def normal(seed, g, q, i):
    """float64 standard normals for (seed, global agent id g, generation q, flat element indices i)"""
    i = np.asarray(i, dtype=np.uint64)
    seed = int(seed)
    x = NR.philox_blocks(np.uint64(g), np.uint64(q), i >> np.uint64(2), np.uint64(TAG), seed & MASK, (seed >> 32) & MASK)
    hi = (i & np.uint64(2)) != 0
    x0, x1 = np.where(hi, x[2], x[0]), np.where(hi, x[3], x[1])
    u0 = ((x0 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u1 = ((x1 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u0))
    ang = 2.0 * np.pi * u1
    return np.where((i & np.uint64(1)) != 0, r * np.sin(ang), r * np.cos(ang))


def perturbed_flat(clean_flat, sigma, seed, g, q):
    """clean_flat: the flat fp32 parameters -> float64 [numel]: w + (float32)sigma * z"""
    w = np.asarray(clean_flat, dtype=np.float32).astype(np.float64)
    return w + float(np.float32(sigma)) * normal(seed, g, q, np.arange(w.size))


def actor_out(params, x):
    """tanh(W3 relu(W2 relu(W1 x + b1) + b2) + b3) in float64; params {name: array}, x [D]"""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    h1 = np.maximum(p['W1'] @ np.asarray(x, dtype=np.float64) + p['b1'], 0.0)
    h2 = np.maximum(p['W2'] @ h1 + p['b2'], 0.0)
    return np.tanh(p['W3'] @ h2 + p['b3'])


def action_distance(clean, noisy, x):
    """ddpg_agent.py:173-175 / param_noise.py:59-63: the L2 distance of the two actors' outputs on x"""
    d = actor_out(noisy, x) - actor_out(clean, x)
    return float(np.sqrt(np.sum(d * d)))


def adapt(sigma, dist, acts, target, alpha):
    """param_noise.py:65-70 with Python's own float operations"""
    sigma, dist = float(sigma), float(dist)
    return sigma / alpha if dist / acts > target else sigma * alpha
