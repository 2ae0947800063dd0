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
    done   = t + 1 >= episode_len (the environment's clock; on done the actor restarts from its init_state)
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
