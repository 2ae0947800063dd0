"""
Episode clocks per actor for the one-launch rollouts (struct smx_actor_clock_rows, include/surreal_amd.h).  Actor a has
an episode length L[a] >= 1 and a clock t[a] in [0, L[a]); a step at clock tau ends the episode when tau + 1 >= L[a]
(the clock restarts at 0) and closes a record -- a moving window of n_step steps, `advance` apart, or with advance 1
an n-step transition -- iff j = tau + 1 - n_step >= 0 and j % advance == 0.  What the host needs of a call of `steps`
steps is a pure function of the clocks, in closed form, so nothing is read back from the device:

  * ``closings``  -- how many records each actor closes;
  * ``after``     -- the clocks after the call;
  * ``row_table`` -- brute force, for doubles and tests: where every closing (step, actor) pair goes, numbered in
    (step, actor) order -- the order in which n host wrappers stepped in actor order insert.
"""
import numpy as np


def _closed_by(x, n_step, advance):
    """records whose closing step tau has tau + 1 <= x, since the episode's start: tau + 1 = n_step, n_step + advance, ..."""
    return np.where(x >= n_step, (x - n_step) // advance + 1, 0)


def _clocks(t, L):
    t, L = np.asarray(t, dtype=np.int64), np.asarray(L, dtype=np.int64)
    if t.shape != L.shape or t.ndim != 1:
        raise ValueError('actor clocks: t %s and episode lengths %s must be two [n] arrays' % (t.shape, L.shape))
    if (L < 1).any() or (t < 0).any() or (t >= L).any():
        raise ValueError('actor clocks: every episode length must be >= 1 and every clock in [0, length)')
    return t, L


def closings(t, L, steps, n_step, advance):
    """-> int64 [n]: the records actor a closes in `steps` steps from clock t[a]: the rest of its open episode, the whole
    episodes behind it, the one it has begun"""
    t, L = _clocks(t, L)
    m = np.minimum(steps, L - t)
    r = steps - m
    f = lambda x: _closed_by(x, n_step, advance)  # noqa: E731
    return f(t + m) - f(t) + (r // L) * f(L) + f(r % L)


def after(t, L, steps):
    """-> int32 [n]: the clocks after `steps` steps"""
    t, L = _clocks(t, L)
    return ((t + steps) % L).astype(np.int32)


def row_table(t, L, steps, n_step, advance):
    """-> (int32 [steps, n], rows): the number of every closing (step, actor) pair in (step, actor) order, -1 where the
    pair closes nothing; a walk over all pairs"""
    t, L = _clocks(t, L)
    tau = t.copy()
    table = np.full((steps, t.size), -1, dtype=np.int32)
    rows = 0
    for s in range(steps):
        for a in range(t.size):
            j = tau[a] + 1 - n_step
            if j >= 0 and j % advance == 0:
                table[s, a] = rows
                rows += 1
            tau[a] = 0 if tau[a] + 1 >= L[a] else tau[a] + 1
    return table, rows
