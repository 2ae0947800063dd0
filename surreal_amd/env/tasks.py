"""
The dynamics the synthetic environments can run, by name ('drift' | 'reach'), and the one host definition of `reach`.

'drift' (synthetic_env.py's docstring) is a fixed workload: every state element decays on its own and no policy is
meaningfully better than another.  'reach' is a task: J point masses are steered to J goals, A = J, D = 3 J, the state
row is [p (J) | v (J) | g (J)] -- position, velocity, goal -- and the policy observes the row itself.

All arithmetic is fp32 with no fused multiply-add, each product rounded before the sum, in exactly this order (the
device's reach_* functions of csrc/smx_synth_env.inc.h evaluate the same expressions, so host and device agree bit for
bit):

    a      = clip(action, -1, 1)
    v'[j]  = clamp((0.9f * v[j]) + (0.2f * a[j]), -1, 1)
    p'[j]  = clamp(p[j] + (0.1f * v'[j]), -10, 10)
    g'[j]  = g[j]
    d[j]   = p'[j] - g[j]
    reward = (float)(-(sum_j (double)d[j] (double)d[j]  +  0.01 sum_j (double)a[j] (double)a[j]))
             both sums in fp64, j ascending, one term at a time, rounded once
    done   = t + 1 >= episode_len (the environment's clock; on done the actor restarts from its init_state, or -- with a
             reset stream, reach_reset_state below -- from a row drawn for its next episode)
"""
import numpy as np

from surreal_amd import _lib as L

TASKS = ('drift', 'reach')
TASK_IDS = {'drift': L.SMX_TASK_DRIFT, 'reach': L.SMX_TASK_REACH}

REACH_MAX_A = 21                             # D = 3 A <= 63: a row's elements sit in one wavefront
REACH_V_DECAY = np.float32(0.9)
REACH_V_GAIN = np.float32(0.2)
REACH_DT = np.float32(0.1)
REACH_V_MAX = np.float32(1.0)
REACH_P_MAX = np.float32(10.0)
REACH_ACTION_COST = 0.01
REACH_PD_KP = np.float32(4.0)
REACH_PD_KD = np.float32(2.0)


def check_task(who, task, obs_dim, action_dim, pixel=None):
    """what both synthetic environments ask of a task and its shapes"""
    if task not in TASKS:
        raise ValueError('%s: task must be one of %r, got %r' % (who, TASKS, task))
    if task == 'reach':
        if obs_dim != 3 * action_dim:
            raise ValueError("%s: task 'reach' has obs_dim == 3 * action_dim (position | velocity | goal), got "
                             'obs_dim %d, action_dim %d' % (who, obs_dim, action_dim))
        if pixel is not None:
            raise ValueError("%s: task 'reach' has no camera" % who)


def reach_step(state, action):
    """state [..., 3 J] and action [..., J] -> (next_state [..., 3 J] fp32, reward [...] fp32): one step of `reach`
    (the module docstring's expressions; no clock and no reset -- those are the environment's)"""
    s = np.asarray(state, dtype=np.float32)
    a = np.clip(np.asarray(action, dtype=np.float32), -1.0, 1.0).astype(np.float32)
    J = a.shape[-1]
    assert s.shape[-1] == 3 * J and s.shape[:-1] == a.shape[:-1], (s.shape, a.shape)
    p, v, g = s[..., :J], s[..., J:2 * J], s[..., 2 * J:]
    vn = ((REACH_V_DECAY * v).astype(np.float32) + (REACH_V_GAIN * a).astype(np.float32)).astype(np.float32)
    vn = np.clip(vn, -REACH_V_MAX, REACH_V_MAX).astype(np.float32)
    pn = (p + (REACH_DT * vn).astype(np.float32)).astype(np.float32)
    pn = np.clip(pn, -REACH_P_MAX, REACH_P_MAX).astype(np.float32)
    d = (pn - g).astype(np.float32)
    d64, a64 = d.astype(np.float64), a.astype(np.float64)
    sd = np.zeros(s.shape[:-1], dtype=np.float64)
    sa = np.zeros(s.shape[:-1], dtype=np.float64)
    for j in range(J):                       # (a loop, not numpy's pairwise sum: the device's order)
        sd = sd + d64[..., j] * d64[..., j]
        sa = sa + a64[..., j] * a64[..., j]
    reward = (-(sd + REACH_ACTION_COST * sa)).astype(np.float32)
    return np.concatenate([pn, vn, g], axis=-1).astype(np.float32), reward


def reach_pd_action(state):
    """the controller that solves `reach`: a = 4 (g - p) - 2 v (reach_step clips it)"""
    s = np.asarray(state, dtype=np.float32)
    J = s.shape[-1] // 3
    p, v, g = s[..., :J], s[..., J:2 * J], s[..., 2 * J:]
    return (REACH_PD_KP * (g - p) - REACH_PD_KD * v).astype(np.float32)


# ---- the reset distribution of `reach` (struct smx_reset_stream; csrc/smx_philox.inc.h restates it) ---------------------
# For a seed (64 bits), a global actor id g < 2^32, an episode index e (int64 >= 0) and element k < 3 J of the row:
#     x[0..3] = Philox4x32-10(counter = (g, low32(e), high32(e), 0x52530000 | (k >> 2)), key = (low32(seed), high32(seed)))
#     w       = x[k & 3]
#     u       = (float)(w >> 8) * 0x1p-23f - 1.0f     a 24-bit integer, scaled, minus one: every step exact in fp32
#     state[k] = u      for a position (k < J) or a goal (k >= 2 J):  uniform on the 2^24 multiples of 2^-23 in [-1, 1)
#     state[k] = +0.0f  for a velocity
# The fourth counter word keeps these blocks apart from the exploration stream's (j >> 2 < 16) and the parameter noise's
# (0x504E0001), whatever the seed.  No transcendental function, no rounding: integer numpy and one exact conversion, the
# device's bits.
RESET_TAG = 0x52530000
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter [..., 4] and key [..., 2] (broadcast against each other; integers < 2^32) -> [..., 4] uint32: the ten
    rounds of Philox4x32 (Salmon et al. 2011), in uint64 numpy"""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0               # (32 x 32 bits: no overflow in 64)
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def reach_reset_state(seed, actor, episode, J):
    """-> [3 J] fp32: the row [p | v | g] that global actor `actor` begins episode `episode` with under `seed` (the
    expressions above; actor and episode may be arrays that broadcast: -> [..., 3 J])"""
    seed, J = int(seed), int(J)
    g = np.asarray(actor, dtype=np.int64)
    e = np.asarray(episode, dtype=np.int64)
    if not 0 <= seed < 1 << 64:
        raise ValueError('reach_reset_state: seed must fit 64 bits, got %r' % (seed,))
    if (g < 0).any() or (g >= 1 << 32).any() or (e < 0).any():
        raise ValueError('reach_reset_state: actor ids in [0, 2^32) and episodes >= 0, got %r, %r' % (actor, episode))
    g, e = np.broadcast_arrays(g.astype(np.uint64), e.astype(np.uint64))
    k = np.arange(3 * J, dtype=np.uint64)
    counter = np.stack(np.broadcast_arrays(g[..., None], e[..., None] & _M32, e[..., None] >> np.uint64(32),
                                           np.uint64(RESET_TAG) | (k >> np.uint64(2))), axis=-1)
    x = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))     # [..., 3 J, 4]
    w = np.take_along_axis(x, (k & np.uint64(3)).astype(np.int64).reshape((1,) * g.ndim + (-1, 1)), axis=-1)[..., 0]
    u = ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)).astype(np.float32)
    u[..., J:2 * J] = np.float32(0.0)
    return u
