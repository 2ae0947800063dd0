"""
The dynamics the synthetic environments can run, by name ('drift' | 'reach' | 'arm'), and the one host definition of
`reach` and of `arm`.

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

'arm' is a planar arm of J links: A = J, D = 2 J + 2 (1 <= J <= 30), the state row is [theta (J) | omega (J) | g (2)] --
each link's absolute orientation, its angular velocity, the goal of the fingertip -- and the policy observes the row
itself.  The kinematics are nonlinear and the reward couples every joint through the fingertip.  The same rule of
arithmetic (the device's arm_* functions restate it):

    a         = clip(action, -1, 1)
    omega'[j] = clamp((0.9f * omega[j]) + (0.4f * a[j]), -1, 1)
    theta'[j] = clamp(theta[j] + (0.2f * omega'[j]), -PI_F, PI_F)      PI_F = 3.1415927f: joint limits, no wrap
    x2        = theta'[j] * theta'[j]
    s[j]      = theta'[j] * P_S(x2)     P_S, P_C: Horner from the highest coefficient, acc = (acc * x2) + c_k, each
    c[j]      = P_C(x2)                 operation rounded; c_k = (float)((-1)^k / (2k+1)!), k = 0..8, resp.
                                        (float)((-1)^k / (2k)!), k = 0..9.  The polynomials ARE the definition: no
                                        library sine or cosine (within 1e-6 of them on [-pi, pi]), no division
    g'        = g
    w         = 2^-ceil(log2 J)         a power of two (J = 1: 1): every link has length w, the reach J w is in (0.5, 1]
    dx        = (sum_j (double)c[j]) * w - (double)g[0]        the sums in fp64, j ascending, one term at a time
    dy        = (sum_j (double)s[j]) * w - (double)g[1]
    reward    = (float)(-((dx dx + dy dy) + 0.01 sum_j (double)a[j] (double)a[j]))
    done      = the environment's clock, as for reach; with a reset stream the next episode's row is arm_reset_state's

A reset stream may carry a DISTURBANCE of scale s (fp32, 0 <= s <= 1; `disturbance` below): step t of episode e of global
actor g then adds s * w[j] to the sum that becomes v'[j] resp. omega'[j], the product rounded before the sum, inside the
clamp -- everything downstream of v' / omega' is unchanged:

    reach:  v'[j]     = clamp(((0.9f * v[j]) + (0.2f * a[j])) + (s * w[j]), -1, 1)
    arm:    omega'[j] = clamp(((0.9f * omega[j]) + (0.4f * a[j])) + (s * w[j]), -1, 1)

With s == 0 the term is NOT added (no `+ 0`): a stream without a disturbance leaves the bytes above, signed zeros included.
"""
import math

import numpy as np

from surreal_amd import _lib as L

TASKS = ('drift', 'reach', 'arm')
TASK_IDS = {'drift': L.SMX_TASK_DRIFT, 'reach': L.SMX_TASK_REACH, 'arm': L.SMX_TASK_ARM}

REACH_MAX_A = 21                             # D = 3 A <= 63: a row's elements sit in one wavefront
REACH_V_DECAY = np.float32(0.9)
REACH_V_GAIN = np.float32(0.2)
REACH_DT = np.float32(0.1)
REACH_V_MAX = np.float32(1.0)
REACH_P_MAX = np.float32(10.0)
REACH_ACTION_COST = 0.01
REACH_PD_KP = np.float32(4.0)
REACH_PD_KD = np.float32(2.0)

ARM_MAX_A = 30                               # D = 2 A + 2 <= 62: a row's elements sit in one wavefront
ARM_W_DECAY = np.float32(0.9)
ARM_W_GAIN = np.float32(0.4)
ARM_DT = np.float32(0.2)
ARM_W_MAX = np.float32(1.0)
ARM_PI = np.float32(3.1415927)
ARM_ACTION_COST = 0.01
ARM_RESET_THETA = np.float32(1.0)            # theta = u: in [-1, 1), well inside the limits
ARM_RESET_GOAL = np.float32(0.25)            # g = u / 4: |g| < 0.36 < 0.5 < J w, reachable for every J >= 2
ARM_JT_KP = np.float32(8.0)
ARM_JT_KD = np.float32(2.0)
ARM_SIN_C = tuple(np.float32((-1) ** k / math.factorial(2 * k + 1)) for k in range(9))
ARM_COS_C = tuple(np.float32((-1) ** k / math.factorial(2 * k)) for k in range(10))

# the widest action a task takes on the device (None: no limit of the task's own)
MAX_A = {'drift': None, 'reach': REACH_MAX_A, 'arm': ARM_MAX_A}


def check_task(who, task, obs_dim, action_dim, pixel=None):
    """what both synthetic environments ask of a task and its shapes"""
    if task not in TASKS:
        raise ValueError('%s: task must be one of %r, got %r' % (who, TASKS, task))
    if task == 'arm':
        if obs_dim != 2 * action_dim + 2:
            raise ValueError("%s: task 'arm' has obs_dim == 2 * action_dim + 2 (orientation | angular velocity | goal), "
                             'got obs_dim %d, action_dim %d' % (who, obs_dim, action_dim))
        if pixel is not None:
            raise ValueError("%s: task 'arm' has no camera" % who)
    if task == 'reach':
        if obs_dim != 3 * action_dim:
            raise ValueError("%s: task 'reach' has obs_dim == 3 * action_dim (position | velocity | goal), got "
                             'obs_dim %d, action_dim %d' % (who, obs_dim, action_dim))
        if pixel is not None:
            raise ValueError("%s: task 'reach' has no camera" % who)


def _disturb(who, vn, w, scale):
    """the sum that becomes v' / omega' with the step's disturbance: vn + (scale * w), or vn itself where scale == 0"""
    scale = np.float32(scale)
    if not 0.0 <= float(scale) <= 1.0:
        raise ValueError('%s: the disturbance scale lies in [0, 1], got %r' % (who, float(scale)))
    if scale == 0:
        return vn
    if w is None:
        raise ValueError('%s: a disturbed step takes its draws w (tasks.disturbance)' % who)
    w = np.asarray(w, dtype=np.float32)
    assert w.shape == vn.shape, (w.shape, vn.shape)
    return (vn + (scale * w).astype(np.float32)).astype(np.float32)


def reach_step(state, action, w=None, scale=0.0):
    """state [..., 3 J] and action [..., J] -> (next_state [..., 3 J] fp32, reward [...] fp32): one step of `reach`
    (the module docstring's expressions; no clock and no reset -- those are the environment's).  scale != 0: a disturbed
    step, w [..., J] its draws (`disturbance`)"""
    s = np.asarray(state, dtype=np.float32)
    a = np.clip(np.asarray(action, dtype=np.float32), -1.0, 1.0).astype(np.float32)
    J = a.shape[-1]
    assert s.shape[-1] == 3 * J and s.shape[:-1] == a.shape[:-1], (s.shape, a.shape)
    p, v, g = s[..., :J], s[..., J:2 * J], s[..., 2 * J:]
    vn = ((REACH_V_DECAY * v).astype(np.float32) + (REACH_V_GAIN * a).astype(np.float32)).astype(np.float32)
    vn = _disturb('reach_step', vn, w, scale)
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


# ---- the per-step disturbance (struct smx_reset_stream's scale; csrc/smx_philox.inc.h restates it) ------------------------------
# For a seed, a global actor id g < 2^32, the episode under way e (0 <= e < 2^32), the step t within it (0 <= t < 2^32) and
# joint / mass j < J:
#     x[0..3] = Philox4x32-10(counter = (g, low32(e), t, 0x44530000 | (j >> 2)), key = (low32(seed), high32(seed)))
#     w[j]    = (float)(x[j & 3] >> 8) * 0x1p-23f - 1.0f       the reset stream's exact conversion: w in [-1, 1)
# The tag keeps these blocks apart from the reset blocks (RESET_TAG), the exploration stream's (fourth word < 16) and the
# parameter noise's (0x504E0001).  The draw is a pure function of (seed, g, e, t, j): not of how a run is cut into calls, of
# the block size or of how the actors are split over envs.
DISTURB_TAG = 0x44530000


def check_disturbance(who, scale):
    """-> the scale as np.float32; a scale outside [0, 1] (a NaN too) is a ValueError"""
    try:
        s = np.float32(scale)
    except (TypeError, ValueError):
        raise ValueError('%s: the disturbance scale is a number in [0, 1], got %r' % (who, scale))
    if not 0.0 <= float(s) <= 1.0:
        raise ValueError('%s: the disturbance scale lies in [0, 1], got %r' % (who, scale))
    return s


def disturbance(seed, actor, episode, t, J):
    """-> [..., J] fp32: w of step `t` of episode `episode` of global actor `actor` under `seed` (the expressions above;
    actor, episode and t may be arrays that broadcast)"""
    seed, J = int(seed), int(J)
    g = np.asarray(actor, dtype=np.int64)
    e = np.asarray(episode, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    if not 0 <= seed < 1 << 64:
        raise ValueError('disturbance: seed must fit 64 bits, got %r' % (seed,))
    if any((v < 0).any() or (v >= 1 << 32).any() for v in (g, e, t)):
        raise ValueError('disturbance: actor ids, episodes and steps in [0, 2^32), got %r, %r, %r' % (actor, episode, t))
    g, e, t = np.broadcast_arrays(g.astype(np.uint64), e.astype(np.uint64), t.astype(np.uint64))
    j = np.arange(J, dtype=np.uint64)
    counter = np.stack(np.broadcast_arrays(g[..., None], e[..., None], t[..., None],
                                           np.uint64(DISTURB_TAG) | (j >> np.uint64(2))), axis=-1)
    x = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))     # [..., J, 4]
    w = np.take_along_axis(x, (j & np.uint64(3)).astype(np.int64).reshape((1,) * g.ndim + (-1, 1)), axis=-1)[..., 0]
    return ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)).astype(np.float32)


# ---- `arm` (the module docstring's expressions) --------------------------------------------------------------------------
def arm_link(J):
    """w = 2^-ceil(log2 J): the length of each of the J links"""
    J = int(J)
    assert J >= 1, J
    return 2.0 ** -((J - 1).bit_length())


def _horner(x2, coef):
    acc = np.full_like(x2, coef[-1])
    for c in coef[-2::-1]:
        acc = ((acc * x2).astype(np.float32) + c).astype(np.float32)
    return acc


def arm_sincos(theta):
    """theta fp32 -> (s, c) fp32: the task's sine and cosine, the two polynomials in theta^2 (for |theta| <= PI_F)"""
    x = np.asarray(theta, dtype=np.float32)
    x2 = (x * x).astype(np.float32)
    return (x * _horner(x2, ARM_SIN_C)).astype(np.float32), _horner(x2, ARM_COS_C)


def _arm_tip(s, c, J):
    """(x, y) fp64 of the fingertip from the links' sines and cosines [..., J]: sums j ascending, one term at a time"""
    sx = np.zeros(s.shape[:-1], dtype=np.float64)
    sy = np.zeros(s.shape[:-1], dtype=np.float64)
    for j in range(J):
        sx = sx + c[..., j].astype(np.float64)
        sy = sy + s[..., j].astype(np.float64)
    w = arm_link(J)
    return sx * w, sy * w


def arm_step(state, action, w=None, scale=0.0):
    """state [..., 2 J + 2] and action [..., J] -> (next_state [..., 2 J + 2] fp32, reward [...] fp32): one step of `arm`
    (no clock and no reset -- those are the environment's).  scale != 0: a disturbed step, w [..., J] its draws
    (`disturbance`)"""
    st = np.asarray(state, dtype=np.float32)
    a = np.clip(np.asarray(action, dtype=np.float32), -1.0, 1.0).astype(np.float32)
    J = a.shape[-1]
    assert st.shape[-1] == 2 * J + 2 and st.shape[:-1] == a.shape[:-1], (st.shape, a.shape)
    th, om, g = st[..., :J], st[..., J:2 * J], st[..., 2 * J:]
    on = ((ARM_W_DECAY * om).astype(np.float32) + (ARM_W_GAIN * a).astype(np.float32)).astype(np.float32)
    on = _disturb('arm_step', on, w, scale)
    on = np.clip(on, -ARM_W_MAX, ARM_W_MAX).astype(np.float32)
    tn = (th + (ARM_DT * on).astype(np.float32)).astype(np.float32)
    tn = np.clip(tn, -ARM_PI, ARM_PI).astype(np.float32)
    s, c = arm_sincos(tn)
    x, y = _arm_tip(s, c, J)
    dx = x - g[..., 0].astype(np.float64)
    dy = y - g[..., 1].astype(np.float64)
    a64 = a.astype(np.float64)
    sa = np.zeros(st.shape[:-1], dtype=np.float64)
    for j in range(J):
        sa = sa + a64[..., j] * a64[..., j]
    reward = (-((dx * dx + dy * dy) + ARM_ACTION_COST * sa)).astype(np.float32)
    return np.concatenate([tn, on, g], axis=-1).astype(np.float32), reward


def arm_jt_action(state):
    """the Jacobian-transpose baseline of `arm`: a_j = -8 (-s_j ex + c_j ey) - 2 omega_j, e = tip - g at the state's own
    orientations (arm_step clips it); what reach_pd_action is to `reach`"""
    st = np.asarray(state, dtype=np.float32)
    J = (st.shape[-1] - 2) // 2
    th, om, g = st[..., :J], st[..., J:2 * J], st[..., 2 * J:]
    s, c = arm_sincos(th)
    x, y = _arm_tip(s, c, J)
    ex = (x - g[..., 0].astype(np.float64))[..., None]
    ey = (y - g[..., 1].astype(np.float64))[..., None]
    return (-float(ARM_JT_KP) * (-s.astype(np.float64) * ex + c.astype(np.float64) * ey)
            - float(ARM_JT_KD) * om.astype(np.float64)).astype(np.float32)


def _reset_uniform(who, seed, actor, episode, width):
    """-> [..., width] fp32: u of elements k < width of the reset stream's row (the expressions above `philox4x32_10`)"""
    seed = int(seed)
    g = np.asarray(actor, dtype=np.int64)
    e = np.asarray(episode, dtype=np.int64)
    if not 0 <= seed < 1 << 64:
        raise ValueError('%s: seed must fit 64 bits, got %r' % (who, seed))
    if (g < 0).any() or (g >= 1 << 32).any() or (e < 0).any():
        raise ValueError('%s: actor ids in [0, 2^32) and episodes >= 0, got %r, %r' % (who, actor, episode))
    g, e = np.broadcast_arrays(g.astype(np.uint64), e.astype(np.uint64))
    k = np.arange(width, dtype=np.uint64)
    counter = np.stack(np.broadcast_arrays(g[..., None], e[..., None] & _M32, e[..., None] >> np.uint64(32),
                                           np.uint64(RESET_TAG) | (k >> np.uint64(2))), axis=-1)
    x = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    w = np.take_along_axis(x, (k & np.uint64(3)).astype(np.int64).reshape((1,) * g.ndim + (-1, 1)), axis=-1)[..., 0]
    return ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)).astype(np.float32)


def arm_reset_state(seed, actor, episode, J):
    """-> [2 J + 2] fp32: the row [theta | omega | g] that global actor `actor` begins episode `episode` with under `seed`
    -- reach's stream, blocks and tag (word k & 3 of block k >> 2 serves element k): theta[j] = 1.0f * u, omega[j] = +0, g[i] = 0.25f * u (exact); actor and episode may be arrays that broadcast: -> [..., 2 J + 2]"""
    J = int(J)
    u = _reset_uniform('arm_reset_state', seed, actor, episode, 2 * J + 2)
    u[..., :J] = (ARM_RESET_THETA * u[..., :J]).astype(np.float32)
    u[..., J:2 * J] = np.float32(0.0)
    u[..., 2 * J:] = (ARM_RESET_GOAL * u[..., 2 * J:]).astype(np.float32)
    return u


# per task: one step, the reset stream's row (None: no reset distribution), the baseline controller
STEP = {'reach': reach_step, 'arm': arm_step}
RESET_STATE = {'reach': reach_reset_state, 'arm': arm_reset_state}
BASELINE_ACTION = {'reach': reach_pd_action, 'arm': arm_jt_action}
