"""
The `arm` task (surreal_amd/env/tasks.py) on the host and on the device, shared by the CPU tier (test_arm_cpu.py) and the
GPU tier (test_gpu_arm.py, test_gpu_arm_learning.py).  Built on reach_cases (agents, calls, episodes, bounds, margins):

  * ``ArmEnv``        -- the float64 restatement of the task with the ``step()`` interface of ``rollout_fp64_ref.Env``.
    Written from the definition -- the two Taylor polynomials with their exact rational coefficients, evaluated in
    float64 --; it calls nothing from surreal_amd.  It keeps how close a clamp's argument came to its bound;
  * ``ArmCpuKernels`` -- the torch-CPU double of the task: the reach / resets / DDPG-variants doubles composed
    (reach_ddpg_variants_cases.ReachVariantsCpuKernels) with the task's step and reset row in place of reach's, both the
    host definition itself (tasks.arm_step, tasks.arm_reset_state), so the CPU tier compares bit for bit;
  * ``Case`` / ``setup`` / ``run`` / ``restatement`` -- reach_cases' on task 'arm'; ``tuned``: the seed per case under
    which the restatement ALONE keeps every ReLU pre-activation, action clip and environment clamp MARGIN from its kink
    (``python tests/arm_cases.py`` prints the entries that differ from the case's own).
"""
import contextlib
import math

import numpy as np
import torch

import reach_cases as RC
import reach_cpu_kernels as RK
import reach_ddpg_variants_cases as RV
import reach_resets_cpu_kernels as RRK
import rollout_envelope_cases as EC
import rollout_fp64_ref as R
from surreal_amd.env import tasks as TK

EP, CALLS = 5, (7, 6)             # T = 13 over episodes of 5: two episode ends inside, the second call starts mid-episode
N_STEP, STRIDE, GAMMA, MARGIN, SEED = RC.N_STEP, RC.STRIDE, RC.GAMMA, RC.MARGIN, RC.SEED
RSEED = 0x5DEECE66D1234567
PI_F = float(np.float32(3.1415927))
C_WDECAY, C_WGAIN, C_DT = (float(np.float32(v)) for v in (0.9, 0.4, 0.2))      # the definition's fp32 constants, upcast
C_COST = 0.01
SIN_C = [(-1.0) ** k / math.factorial(2 * k + 1) for k in range(9)]
COS_C = [(-1.0) ** k / math.factorial(2 * k) for k in range(10)]


def obs_dim(J):
    return 2 * J + 2


def link(J):
    """2^-ceil(log2 J)"""
    w = 1.0
    while 1.0 / w < J:
        w *= 0.5
    return w


def poly(x2, coef):
    acc = torch.full_like(x2, coef[-1])
    for c in coef[-2::-1]:
        acc = acc * x2 + c
    return acc


class ArmEnv(R.Env):
    """[theta | omega | g]: omega' = clamp(0.9 omega + 0.4 a, +-1); theta' = clamp(theta + 0.2 omega', +-PI_F); tip =
    w (sum cos theta', sum sin theta'); reward = -(|tip - g|^2 + 0.01 sum a^2); done = t + 1 >= episode_len; a done actor
    restarts from its initial state, the clock from 0"""

    def __init__(self, init_state, A, episode_len, state=None, t=0):
        super().__init__(init_state, A, episode_len, state, t)
        assert self.D == 2 * self.A + 2
        self.clip_margin = float('inf')       # min over steps and links of | |argument| - bound | of the two clamps

    def step(self, actions):
        J = self.A
        a = torch.clamp(actions, -1.0, 1.0)
        s = self.state
        th, om, g = s[:, :J], s[:, J:2 * J], s[:, 2 * J:]
        orr = C_WDECAY * om + C_WGAIN * a
        on = torch.clamp(orr, -1.0, 1.0)
        tr = th + C_DT * on
        tn = torch.clamp(tr, -PI_F, PI_F)
        self.clip_margin = min(self.clip_margin, float((orr.abs() - 1.0).abs().min()), float((tr.abs() - PI_F).abs().min()))
        x2 = tn * tn
        sn_, cs_ = tn * poly(x2, SIN_C), poly(x2, COS_C)
        w = link(J)
        dx, dy = cs_.sum(1) * w - g[:, 0], sn_.sum(1) * w - g[:, 1]
        rew = -((dx * dx + dy * dy) + C_COST * (a * a).sum(1))
        sn = torch.cat([tn, on, g], 1)
        done = self.t + 1 >= self.L
        self.ep_sum, self.ep_abs, self.ep_len = self.ep_sum + rew, self.ep_abs + rew.abs(), self.ep_len + 1
        if done:
            self.finished.append((self.ep_sum, self.ep_abs, self.ep_len))
            self.ep_sum, self.ep_abs, self.ep_len = torch.zeros_like(rew), torch.zeros_like(rew), 0
        self.state = self.init.clone() if done else sn
        self.t = 0 if done else self.t + 1
        return s, sn, rew, done


# ---- the double ------------------------------------------------------------------------------------------------------------

def arm(state, acts):
    """arm_step on torch fp32 tensors -> (next state before any reset, reward)"""
    sn, rew = TK.arm_step(state.detach().cpu().numpy(), acts.detach().cpu().numpy())
    return torch.as_tensor(sn), torch.as_tensor(rew)


def drawn(resets, n, J, ahead=0):
    """[n, 2 J + 2] fp32: the rows of episode resets[2] + ahead for the actors resets[1] .. resets[1] + n - 1"""
    seed, base, episode = (int(v) for v in resets)
    return torch.as_tensor(TK.arm_reset_state(seed, base + np.arange(n), episode + ahead, J))


class ArmCpuKernels(RV.ReachVariantsCpuKernels):
    """With task 'arm' a call runs the doubles it inherits as they run 'reach' -- the same clocks, windows, n-step sums,
    monitor feeds and reset hooks -- with the step and the drawn row they call replaced by arm's for the length of the
    call; every other task goes to them untouched."""
    name = 'torch-cpu-double+tasks+resets+ddpg-variants+arm'
    _arm_D = None            # while an arm call runs: the row width

    @contextlib.contextmanager
    def _as_arm(self, D):
        assert D >= 4 and D % 2 == 0, D
        saved = (RK.reach, RRK.drawn, self._arm_D)
        RK.reach, self._arm_D = arm, D
        RRK.drawn = lambda resets, n, J, ahead=0: drawn(resets, n, (D - 2) // 2, ahead)
        try:
            yield
        finally:
            RK.reach, RRK.drawn, self._arm_D = saved

    def synth_task_supported(self, task, D, A):
        if self._arm_D is not None and task == 'reach':
            task = 'arm'
        return super().synth_task_supported(task, D, A)

    def reset_fill(self, resets, out, task='reach'):
        if task != 'arm':
            return super().reset_fill(resets, out, task=task)
        J = (out.shape[1] - 2) // 2
        assert self.synth_task_supported(task, out.shape[1], J)
        out.copy_(drawn(resets, out.shape[0], J))

    def synth_env_step(self, state, *a, task='drift', **kw):
        if task != 'arm':
            return super().synth_env_step(state, *a, task=task, **kw)
        with self._as_arm(state.shape[1]):
            return super().synth_env_step(state, *a, task='reach', **kw)

    def synth_ppo_window_rollout(self, model, packed, lstm_packed, state, *a, task='drift', **kw):
        if task != 'arm':
            return super().synth_ppo_window_rollout(model, packed, lstm_packed, state, *a, task=task, **kw)
        with self._as_arm(state.shape[1]):
            return super().synth_ppo_window_rollout(model, packed, lstm_packed, state, *a, task='reach', **kw)

    def synth_ddpg_rollout(self, net, packed, r, steps, *a, task='drift', **kw):
        if task != 'arm':
            return super().synth_ddpg_rollout(net, packed, r, steps, *a, task=task, **kw)
        with self._as_arm(r['state'].shape[1]):
            try:
                return super().synth_ddpg_rollout(net, packed, r, steps, *a, task='reach', **kw)
            finally:
                self.routes[-1]['task'] = 'arm'


# ---- small cases on a kernels object -----------------------------------------------------------------------------------

Case = RC.Case
# family: 'window' (plain MLP), 'lstm_window' (an LSTM of 10 units in front), 'ddpg' (plain actor, OU noise); hidden sizes
# per case (H1, H2): (32, 32) and the ragged (28, 20).  J = 1 (D = 4), J = 2, J = 30 (D = 62: the row's last lane is lane
# 61).  n = 5: one partial 4-actor block; n = 20: more than one block at every size, a partial one at 8 and 16.
HIDDEN = {}


def _case(cid, family, J, n, H, hidden, scale, streams):
    HIDDEN[cid] = hidden
    return Case(cid, family, obs_dim(J), J, n, H, 0, scale, streams)


CASES = [
    _case('window-J1-n5', 'window', 1, 5, None, (32, 32), 3.0, False),
    _case('window-J2-n20-streams', 'window', 2, 20, None, (28, 20), 3.0, True),
    _case('window-J30-n5', 'window', 30, 5, None, (32, 32), 3.0, False),
    _case('lstm_window-J2-n5-streams', 'lstm_window', 2, 5, 10, (28, 20), 3.0, True),
    _case('lstm_window-J30-n5', 'lstm_window', 30, 5, 10, (32, 32), 3.0, False),
    _case('ddpg-J1-n20', 'ddpg', 1, 20, None, (28, 20), 6.0, False),
    _case('ddpg-J2-n5-streams', 'ddpg', 2, 5, None, (32, 32), 6.0, True),
    _case('ddpg-J30-n5-streams', 'ddpg', 30, 5, None, (32, 32), 6.0, True),
]
TUNED = {
    'window-J2-n20-streams': (246, 3.0),
    'window-J30-n5': (9, 3.0),
    'lstm_window-J2-n5-streams': (88, 3.0),
    'lstm_window-J30-n5': (5, 3.0),
    'ddpg-J1-n20': (8, 6.0),
    'ddpg-J2-n5-streams': (6, 6.0),
    'ddpg-J30-n5-streams': (16, 6.0),
}
# cases for the equalities of bits alone: no seed in 0 .. 3999 keeps this one's restatement MARGIN from every kink
BITS_ONLY = [
    _case('lstm_window-J30-n20', 'lstm_window', 30, 20, 10, (32, 32), 3.0, False),
]


def tuned(c):
    seed, scale = TUNED.get(c.id, (c.seed, c.scale))
    return c._replace(seed=seed, scale=scale)


@contextlib.contextmanager
def _arm_shapes(c, calls=CALLS):
    """reach_cases' (and reach_resets_cases') setup / run with this module's calls, episodes, the case's hidden sizes and
    the task 'arm' where they say 'reach'"""
    saved = (RC.EP, RC.CALLS, RC.H1, RC.H2, RC.setup)
    plain = getattr(RC.setup, 'plain', RC.setup)

    def arm_setup(c_, device, kernels=None, task='arm', wrap=True):
        return plain(c_, device, kernels, task='arm' if task == 'reach' else task, wrap=wrap)
    arm_setup.plain = plain
    RC.EP, RC.CALLS, RC.setup = EP, calls, arm_setup
    RC.H1, RC.H2 = HIDDEN[c.id]
    try:
        yield
    finally:
        RC.EP, RC.CALLS, RC.H1, RC.H2, RC.setup = saved


def closing_steps(c):
    with _arm_shapes(c):
        return RC.closing_steps(c)


def setup(c, device, kernels=None, wrap=True, task='arm'):
    with _arm_shapes(c):
        return RC.setup(c, device, kernels, task=task, wrap=wrap)


def setup_resets(c, device, kernels=None, wrap=False, actor_base=0):
    """setup, then the reset stream (RSEED) attached and episode 0 begun: x.resets"""
    import reach_resets_cases as RR
    saved, RR.RSEED = RR.RSEED, RSEED
    try:
        with _arm_shapes(c):
            return RR.setup(c, device, kernels, wrap=wrap, actor_base=actor_base)
    finally:
        RR.RSEED = saved


def run(x, apw=0, calls=CALLS):
    if x.venv.monitor is None:
        x.venv.attach_monitor(capacity=4)
    with _arm_shapes(x.c, calls):
        return RC.run(x, apw)


def restatement(x):
    """reach_cases.restatement's on ArmEnv -> (want {field: float64}, rows, written mask, the policy: .margins, .env)"""
    c = x.c
    env = ArmEnv(x.venv.init_state, c.A, EP)
    eps = R.f64(x.eps_ref)
    S = sum(CALLS)
    if c.family == 'ddpg':
        m = x.agent.model
        pol = RC.ProbedDdpgPolicy({k: v for k, v in m.actor.views.items()}, c.n, c.A, noise='ou_noise', sigmas=x.sig,
                                  theta=x.agent.theta, dt=x.agent.dt)
        pol.margins = RC.Margins()
        ring, rows, written = R.ddpg_ring(pol, env, eps, S, N_STEP, GAMMA, x.capacity)
    else:
        p, zf, lstm, ns = EC.ppo_reference_inputs(x.agent, c.n)
        pol = RC.ProbedPpoPolicy(p, zf, lstm, ns)
        pol.margins = RC.Margins()
        ring, rows, written = R.ppo_windows(pol, env, eps, S, N_STEP, STRIDE, x.capacity)
    pol.env = env
    return ring, rows, written, pol


input_conditions = RC.input_conditions


def tune(c, seeds=range(1, 200)):
    """-> the first seed under which the restatement meets the input conditions, the case's own first; a streams case with
    twice the margin (reach_cases.tune's reason)"""
    for seed in [c.seed] + list(seeds):
        t = c._replace(seed=seed)
        x = setup(t, 'cpu', ArmCpuKernels(), wrap=False)
        try:
            input_conditions(restatement(x)[3], (2 if c.streams else 1) * MARGIN)
            return seed, c.scale
        except AssertionError:
            continue
    return None


# ---- the checks both tiers run (the CPU tier on the double, the GPU tier on the kernels) -----------------------------------

def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def closings(calls=CALLS):
    """per closing step of the calls, in ring order: (episode, first step of the window / transition, its last step)"""
    t, e, out = 0, 0, []
    for _ in range(sum(calls)):
        if t >= N_STEP - 1 and (t + 1 - N_STEP) % STRIDE == 0:
            out.append((e, t - N_STEP + 1, t))
        t, e = (0, e + 1) if t + 1 >= EP else (t + 1, e)
    return out


def ddpg_closings(calls=CALLS):
    t, e, out = 0, 0, []
    for _ in range(sum(calls)):
        if t >= N_STEP - 1:
            out.append((e, t - N_STEP + 1, t))
        t, e = (0, e + 1) if t + 1 >= EP else (t + 1, e)
    return out


def check_rows(got, x, rows, resets=None, calls=CALLS):
    """(1) every recorded (obs, action, obs_next, reward) row of a ring with rows to spare, fed to the host arm_step,
    reproduces obs_next and reward bit for bit (DDPG: through the n-step sum, formed as nstep_reward forms it); (3) with
    resets = (seed, actor_base) each episode's first row is arm_reset_state's; (4) -> the episodes' fp64 returns, the
    step-order sums of the host rewards, [n][finished episodes] (windows: they cover every step of an episode)"""
    c, n, N = x.c, x.c.n, N_STEP
    first = lambda e: TK.arm_reset_state(resets[0], resets[1] + np.arange(n), e, c.A)  # noqa: E731
    row = lambda k: slice(k * n, (k + 1) * n)  # noqa: E731
    if c.family != 'ddpg':
        cl = closings(calls)
        assert rows == n * len(cl)
        obs = got['obs'].numpy()[:rows].reshape(-1, N, c.D)
        act = got['actions'].numpy()[:rows].reshape(-1, N, c.A)
        rew = got['rewards'].numpy()[:rows].reshape(-1, N)
        nxt = got['obs_next'].numpy()[:rows].reshape(-1, c.D)
        dones = got['dones'].numpy()[:rows].reshape(-1, N)
        assert np.abs(act).max() <= 1.0 and np.isfinite(obs).all()
        returns = {}
        for k, (e, j, tau) in enumerate(cl):
            for u in range(N):
                sn, r = TK.arm_step(obs[row(k), u], act[row(k), u])
                assert bits(sn, obs[row(k), u + 1] if u + 1 < N else nxt[row(k)]), (k, u)
                assert bits(r, rew[row(k), u]), (k, u)
            assert (dones[row(k), :N - 1] == 0).all() and (dones[row(k), N - 1] == float(tau + 1 >= EP)).all()
            if resets is not None and j == 0:
                assert bits(obs[row(k), 0], first(e)), (k, e)
            # windows of 3 steps, 2 apart: window (0-2) then (2-4) of an episode of 5 -- every step once, in order
            new = rew[row(k), (0 if j == 0 else N - STRIDE):].astype(np.float64)
            tot = returns.setdefault(e, np.zeros(n))
            for u in range(new.shape[1]):
                tot += new[:, u]
        assert (EP, N, STRIDE) == (5, 3, 2)
        full = [e for e in returns if (e, EP - N, EP - 1) in cl]
        return [[float(returns[e][a]) for e in full] for a in range(n)]
    cl = ddpg_closings(calls)
    assert rows == n * len(cl)
    f = {k: got[k].numpy()[:rows] for k in ('obs', 'obs_next', 'actions', 'rewards', 'dones')}
    gpow = np.array([pow(GAMMA, e) for e in range(N)])
    chained = summed = 0
    for k, (e, j, tau) in enumerate(cl):
        sn, r = TK.arm_step(f['obs'][row(k)], f['actions'][row(k)])
        if resets is not None and j == 0:
            assert bits(f['obs'][row(k)], first(e)), (k, e)
        if k + 1 < len(cl) and cl[k + 1][:2] == (e, j + 1):
            assert bits(sn, f['obs'][row(k + 1)]), k
            chained += 1
        if k + N - 1 < len(cl) and cl[k + N - 1][:2] == (e, j + N - 1):
            rews, s_last = [], None
            for u in range(N):
                s_last, ru = TK.arm_step(f['obs'][row(k + u)], f['actions'][row(k + u)])
                rews.append(ru)
            assert bits(s_last, f['obs_next'][row(k)]), k
            full = np.zeros((n, tau + 1), np.float32)
            full[:, j:] = np.stack(rews, 1)
            assert bits(RK.np_nstep_sum(full, gpow, N, tau), f['rewards'][row(k)].reshape(-1)), k
            summed += 1
        assert float(f['dones'][row(k)].min()) == float(f['dones'][row(k)].max()) == float(tau + 1 >= EP)
    assert chained >= 4 and summed >= 2
    return None


def monitor_returns(mon, n):
    """the monitor's finished episodes raw, fp64: [n][episodes]"""
    counts, rewards = mon.ep_count.cpu().numpy(), mon.done_reward.cpu().numpy()
    return [[float(rewards[a, e]) for e in range(int(counts[a]))] for a in range(n)]


def split_envs(c, device, kernels=None, apw=0):
    """-> (one env of 8 actors on the reset stream, its ring; [two envs of 4 actors, actor_base 0 and 4, and their
    rings]): reach_resets_cases.split_envs on this module's setup and calls"""
    big = setup_resets(c._replace(n=8), device, kernels)
    gb, _ = run(big, apw)
    small = []
    for base in (0, 4):
        x = setup_resets(c._replace(n=4), device, kernels, actor_base=base)
        if big.eps is not None:
            x.eps = big.eps[:, base:base + 4].contiguous()
        if big.sig is not None:
            x.sig = big.sig[base:base + 4].contiguous()
        else:                                       # (PPO's per-actor noise scales are the agent's: its share of them)
            x.agent.batch_noise = lambda n, s=big.agent.batch_noise(8)[base:base + 4].contiguous(): s
        small.append((x, run(x, apw)[0]))
    return (big, gb), small


def whole_steps(device, kernels=None, n=5, J=2, calls=CALLS, layernorm=False, param_noise=None, apw=0):
    """DDPG with n_step 1 on the reset stream: every step closes, a row is (s, a, r, s') of one step -- n host chains over
    SyntheticEnv(task='arm', resets=...) on the recorded actions give every row, the state left and the episode returns
    layernorm / param_noise ('normal': populations of 4 actors, n a multiple of 4): the actor variants of the launch.
    -> (the monitor's returns, the chains')"""
    import ddpg_rollout_cases as DC
    from surreal_amd import kernels as KN
    from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    prev = KN.set_default_kernels(kernels, device) if kernels is not None else None
    try:
        D, A, S = obs_dim(J), J, sum(calls)
        lc, ec, sc = DC.configs(D, A, n, hidden=(28, 20), n_step=1, noise_type='normal', memory_size=n * S,
                                layernorm=layernorm, param_noise_type=param_noise)
        agent = DC.make_agent(lc, ec, sc)
        kw = dict(kernels=kernels) if kernels is not None else {}
        venv = SyntheticVecEnv(n, D, A, episode_len=EP, device=device, task='arm', **kw)
        mon = venv.attach_monitor(capacity=4)
        venv.attach_resets(RSEED, 3)
        venv.reset()
        if param_noise:
            venv.attach_param_noise(agent, SEED, actors_per_agent=4)
        replay = UniformReplay(lc, ec, sc)
        eps = torch.randn(S, n, A, generator=torch.Generator().manual_seed(5)).to(device)
        s0 = 0
        for T in calls:
            venv.ddpg_rollout_into(agent, replay, T, eps=eps[s0:s0 + T], actors_per_workgroup=apw)
            s0 += T
        f = {k: v.numpy() for k, v in EC.ring_fields(replay, ('obs', 'obs_next', 'actions', 'rewards', 'dones')).items()}
        state = venv.state.detach().cpu().numpy()
        got = monitor_returns(mon, n)
    finally:
        if prev is not None:
            KN.set_default_kernels(*prev)
    flat = lambda o: o['low_dim']['flat_inputs']  # noqa: E731
    returns = []
    for a in range(n):
        h = SyntheticEnv(D, A, episode_len=EP, task='arm', resets=(RSEED, 3 + a))
        o, _ = h._reset()
        returns.append([0.0])
        for s in range(S):
            r_ = s * n + a
            assert bits(flat(o), f['obs'][r_]), (a, s)
            o, r, done, _ = h._step(f['actions'][r_])
            assert bits(flat(o), f['obs_next'][r_]) and bits(np.float32(r), f['rewards'][r_].reshape(-1)[0]), (a, s)
            assert float(f['dones'][r_].reshape(-1)[0]) == float(done)
            returns[-1][-1] += r
            if done:
                o, _ = h._reset()
                returns[-1].append(0.0)
        assert bits(flat(o), state[a])
    return got, [r[:-1] for r in returns]


def host_eval_returns(J, n, E, L, action, resets=None, init_state=None):
    """np.float64 [n, E]: the returns of E episodes of L steps per actor under the constant action `action`, from
    arm_reset_state (resets = (seed, first_episode, actor_base)) or init_state: the fp64 step-order sum of arm_step's fp32
    rewards"""
    out = np.zeros((n, E), dtype=np.float64)
    act = np.full(J, action, dtype=np.float32)
    for a in range(n):
        for i in range(E):
            s = TK.arm_reset_state(resets[0], resets[2] + a, resets[1] + i, J) if resets is not None \
                else np.asarray(init_state[a], dtype=np.float32)
            total = 0.0
            for _ in range(L):
                s, r = TK.arm_step(s, act)
                total = total + float(r)
            out[a, i] = total
    return out


if __name__ == '__main__':          # prints TUNED's entries
    from surreal_amd import kernels as _KN
    _KN.set_default_kernels(ArmCpuKernels(), 'cpu')
    for c_ in CASES:
        got_ = tune(c_)
        if got_ != (c_.seed, c_.scale):
            print('    %r: %r,' % (c_.id, got_), flush=True)
