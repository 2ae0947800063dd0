"""
The per-step disturbance of the tasks `reach` and `arm` (surreal_amd/env/tasks.py: disturbance; struct smx_reset_stream's
scale), shared by the CPU tier (test_task_disturbance_cpu.py) and the GPU tier (test_gpu_task_disturbance.py,
test_gpu_task_disturbance_restatement.py, test_gpu_task_disturbance_learning.py).  Built on reach_cases / reach_resets_cases
and arm_cases (agents, rings, draws):

  * ``DisturbedCpuKernels`` -- the torch-CPU double: arm_cases.ArmCpuKernels (every task double composed) whose three
    stepping doubles take a stream (seed, actor_base, episode, scale).  For the length of such a call the step the doubles
    run -- tasks.reach_step / tasks.arm_step, the host definition -- gets the step's draws, tasks.disturbance(seed, actor,
    the episode under way, the step within it, J), and the scale, so the CPU tier compares bit for bit;
  * ``Case`` / ``setup`` / ``run`` -- a reach or arm case of those modules with the stream re-attached at a scale, stepped over
    CALLS = 3 + 4 + 5 steps of episodes of 5: two episode ends fall inside calls;
  * ``check_rows`` -- every recorded row against the host step with the host draws; ``whole_steps`` -- the four DDPG
    actors with n_step 1 against host chains over SyntheticEnv(..., disturbance=);
  * ``DisturbedReachEnv`` / ``DisturbedArmEnv`` -- the float64 restatements (rollout_fp64_ref's Env interface) with the
    term added in float64; the draws are inputs, exact in float64.
"""
import collections
import contextlib

import numpy as np
import torch

import arm_cases as AC
import ddpg_rollout_cases as DC
import reach_cases as RC
import reach_cpu_kernels as RK
import reach_resets_cases as RR
import rollout_envelope_cases as EC
import rollout_fp64_ref as R
from surreal_amd.env import tasks as TK

EP, CALLS = 5, (3, 4, 5)          # 12 steps over episodes of 5: the ends at steps 4 and 9 fall inside calls two and three
N_STEP, STRIDE, GAMMA = RC.N_STEP, RC.STRIDE, RC.GAMMA
SCALE = float(np.float32(0.3))    # no power of two: the product s * w rounds
SEEDS = {'reach': RR.RSEED, 'arm': AC.RSEED}
assert (RC.EP, AC.EP, sum(RC.CALLS)) == (EP, EP, sum(CALLS))


def obs_dim(task, J):
    return 3 * J if task == 'reach' else 2 * J + 2


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the double ------------------------------------------------------------------------------------------------------------

class DisturbedCpuKernels(AC.ArmCpuKernels):
    name = AC.ArmCpuKernels.name + '+disturbance'
    _dist = None             # while a disturbed call runs: [seed, actor_base, its first episode under way, scale, t, ends]

    @contextlib.contextmanager
    def _disturbing(self, resets, t, steps, episode_len):
        """-> the keywords the inherited double takes for `resets`; a stream with a scale: what the entry points refuse is
        refused, and the host steps draw for the length of the call"""
        if resets is None:
            yield {}
            return
        plain = dict(resets=tuple(int(v) for v in resets[:3]))
        scale = np.float32(resets[3]) if len(resets) > 3 else np.float32(0.0)
        if scale == 0:
            yield plain
            return
        seed, base, episode = plain['resets']
        assert 0.0 < float(scale) <= 1.0, scale
        assert episode >= 1 and episode - 1 + (int(t) + int(steps) - 1) // int(episode_len) < 1 << 32, (episode, t, steps)
        saved = (self._dist, TK.reach_step, TK.arm_step)
        self._dist = q = [seed, base, episode - 1, scale, int(t), 0]

        def drawing(step):
            def disturbed(state, action, w=None, scale=0.0):
                n, J = np.asarray(action).shape
                w = TK.disturbance(q[0], q[1] + np.arange(n), q[2] + q[5], q[4], J)
                return step(state, action, w=w, scale=q[3])
            return disturbed
        TK.reach_step, TK.arm_step = drawing(saved[1]), drawing(saved[2])
        try:
            yield plain
        finally:
            self._dist, TK.reach_step, TK.arm_step = saved

    def _before_step(self):
        """(the resets double's hook, once per step before the step's dynamics) this step's clock and the ends before it"""
        if self._dist is not None and self._rst is not None:
            self._dist[4], self._dist[5] = self._rst[3], self._rst[2]
        super()._before_step()

    def reset_fill(self, resets, out, task='reach'):
        return super().reset_fill(tuple(resets[:3]), out, task=task)

    def synth_env_step(self, state, init_state, actions, t, episode_len, *a, resets=None, **kw):
        with self._disturbing(resets, t, 1, episode_len) as rkw:
            return super().synth_env_step(state, init_state, actions, t, episode_len, *a, **kw, **rkw)

    def synth_ppo_window_rollout(self, model, packed, lstm_packed, state, init_state, noise_scale, eps, t, episode_len, T,
                                 *a, resets=None, **kw):
        with self._disturbing(resets, t, T, episode_len) as rkw:
            return super().synth_ppo_window_rollout(model, packed, lstm_packed, state, init_state, noise_scale, eps, t,
                                                    episode_len, T, *a, **kw, **rkw)

    def synth_ddpg_rollout(self, net, packed, r, steps, *a, resets=None, **kw):
        with self._disturbing(resets, r['t'], steps, r['episode_len']) as rkw:
            try:
                return super().synth_ddpg_rollout(net, packed, r, steps, *a, **kw, **rkw)
            finally:
                if resets is not None:
                    self.routes[-1]['resets'] = tuple(resets)


# ---- the cases -------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple('Case', 'id task base')
# reach J in {1, 2, 5, 21}, arm J in {1, 2, 5, 30}: J = 5 is the first to use a second Philox block, 21 / 30 are the widest
# rows; n = 5: one partial 4-actor block.  Hidden (8, 4) for reach (reach_cases'), (32, 32) or the ragged (28, 20) for arm
# (arm_cases'); the LSTMs of 8 resp. 10 units.


def _reach(family, J, H=None, scale=3.0):
    cid = 'reach-%s-J%d' % (family, J)
    return Case(cid, 'reach', RC.Case(cid, family, 3 * J, J, 5, H, 0, scale, False))


def _arm(family, J, H=None, hidden=(32, 32), scale=3.0):
    cid = 'arm-%s-J%d' % (family, J)
    return Case(cid, 'arm', AC._case(cid, family, J, 5, H, hidden, scale, False))


CASES = [
    _reach('window', 1), _reach('window', 5), _reach('window', 21), _reach('lstm_window', 2, 8),
    _reach('ddpg', 2, scale=6.0), _reach('ddpg', 21, scale=6.0),
    _arm('window', 2, hidden=(28, 20)), _arm('window', 30), _arm('lstm_window', 5, 10),
    _arm('ddpg', 1, hidden=(28, 20), scale=6.0), _arm('ddpg', 5, scale=6.0), _arm('ddpg', 30, scale=6.0),
]
BY_ID = {c.id: c for c in CASES}


def setup(c, device, kernels=None, scale=SCALE, actor_base=0, n=None, seed=None):
    """the case's agent, env, replay (rows to spare) and draws as its module makes them, then the stream attached again
    with `scale` (None: as the module attached it, without the keyword) and episode 0 begun: x.resets, x.task"""
    b = c.base if n is None else c.base._replace(n=n)
    if seed is not None:
        b = b._replace(seed=seed)
    if c.task == 'reach':
        x = RR.setup(b, device, kernels, wrap=False, actor_base=actor_base)
    else:
        x = AC.setup_resets(b, device, kernels, actor_base=actor_base)
    x.task, x.base = c.task, actor_base
    if scale is not None:
        x.resets = x.venv.attach_resets(SEEDS[c.task], actor_base, disturbance=scale)
        x.venv.reset()
    if x.venv.monitor is None:
        x.venv.attach_monitor(capacity=4)
    return x


def run(x, apw=0, calls=CALLS):
    """the calls -> ({field: tensor on the CPU}: the ring in row order, the state, the carried noise / cells; rows)"""
    if x.task == 'reach':
        return RR.run(x, apw, calls)
    return AC.run(x, apw, calls)


def monitor_bytes(x):
    """everything the monitor holds, as bytes"""
    m = x.venv.monitor
    return [t.detach().cpu().contiguous().view(torch.uint8) for t in (m.ep_reward, m.ep_steps, m.ep_count, m.done_reward, m.done_steps)]


def closings(ddpg, calls=CALLS):
    """per closing step of the calls, in ring order: (episode, first step of the window / transition, its last step)"""
    t, e, out = 0, 0, []
    for _ in range(sum(calls)):
        if t >= N_STEP - 1 and (ddpg or (t + 1 - N_STEP) % STRIDE == 0):
            out.append((e, t - N_STEP + 1, t))
        t, e = (0, e + 1) if t + 1 >= EP else (t + 1, e)
    return out


def check_rows(got, x, rows, scale=SCALE, calls=CALLS):
    """every recorded (obs, action, obs_next, reward) row, fed to the host step with the draws the host definition gives for
    its (actor, episode, step), reproduces obs_next and reward bit for bit (DDPG: through the n-step sum, formed as
    nstep_reward forms it); each episode's first row is the reset stream's; -> the episodes' fp64 returns, the step-order
    sums of the recorded rewards, [n][finished episodes] (windows only: they cover every step of an episode; else None)"""
    c, n, N = x.c, x.c.n, N_STEP
    seed, g = SEEDS[x.task], x.base + np.arange(n)
    step, first = TK.STEP[x.task], lambda e: TK.RESET_STATE[x.task](seed, g, e, c.A)  # noqa: E731

    def host(s, a, e, t):
        if scale == 0:
            return step(s, a)
        return step(s, a, w=TK.disturbance(seed, g, e, t, c.A), scale=scale)
    row = lambda k: slice(k * n, (k + 1) * n)  # noqa: E731
    if c.family != 'ddpg':
        cl = closings(False, calls)
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
                sn, r = host(obs[row(k), u], act[row(k), u], e, j + u)
                assert bits(sn, obs[row(k), u + 1] if u + 1 < N else nxt[row(k)]), (k, u)
                assert bits(r, rew[row(k), u]), (k, u)
            assert (dones[row(k), :N - 1] == 0).all() and (dones[row(k), N - 1] == float(tau + 1 >= EP)).all()
            if j == 0:
                assert bits(obs[row(k), 0], first(e)), (k, e)
            # windows of 3 steps, 2 apart: (0-2) then (2-4) of an episode of 5 -- every step once, in order
            new = rew[row(k), (0 if j == 0 else N - STRIDE):].astype(np.float64)
            tot = returns.setdefault(e, np.zeros(n))
            for u in range(new.shape[1]):
                tot += new[:, u]
        assert (EP, N, STRIDE) == (5, 3, 2)
        full = [e for e in returns if (e, EP - N, EP - 1) in cl]
        return [[float(returns[e][a]) for e in full] for a in range(n)]
    cl = closings(True, calls)
    assert rows == n * len(cl)
    f = {k: got[k].numpy()[:rows] for k in ('obs', 'obs_next', 'actions', 'rewards', 'dones')}
    gpow = np.array([pow(GAMMA, e) for e in range(N)])
    chained = summed = 0
    for k, (e, j, tau) in enumerate(cl):
        sn, r = host(f['obs'][row(k)], f['actions'][row(k)], e, j)
        if j == 0:
            assert bits(f['obs'][row(k)], first(e)), (k, e)
        if k + 1 < len(cl) and cl[k + 1][:2] == (e, j + 1):
            assert bits(sn, f['obs'][row(k + 1)]), k
            chained += 1
        if k + N - 1 < len(cl) and cl[k + N - 1][:2] == (e, j + N - 1):
            rews, s_last = [], None
            for u in range(N):
                s_last, ru = host(f['obs'][row(k + u)], f['actions'][row(k + u)], e, j + u)
                rews.append(ru)
            assert bits(s_last, f['obs_next'][row(k)]), k
            full = np.zeros((n, tau + 1), np.float32)
            full[:, j:] = np.stack(rews, 1)
            assert bits(RK.np_nstep_sum(full, gpow, N, tau), f['rewards'][row(k)].reshape(-1)), k
            summed += 1
        assert float(f['dones'][row(k)].min()) == float(f['dones'][row(k)].max()) == float(tau + 1 >= EP)
    assert chained >= 4 and summed >= 2
    return None


def draws_move_the_rows(got, x, rows):
    """the recorded rows are NOT the undisturbed step's: the term is there"""
    c, n = x.c, x.c.n
    if c.family != 'ddpg':
        obs = got['obs'].numpy()[:n].reshape(n, N_STEP, c.D)
        act = got['actions'].numpy()[:n].reshape(n, N_STEP, c.A)
        sn, _ = TK.STEP[x.task](obs[:, 0], act[:, 0])
        return not bits(sn, obs[:, 1])
    f = {k: got[k].numpy() for k in ('obs', 'actions')}
    sn, _ = TK.STEP[x.task](f['obs'][:n], f['actions'][:n])
    return not bits(sn, f['obs'][n:2 * n])


def split_envs(c, device, kernels=None, apw=0, scale=SCALE):
    """-> (one env of 8 actors, its ring; [two envs of 4 actors, actor_base 0 and 4, and their rings])"""
    big = setup(c, device, kernels, scale, n=8)
    gb, rows = run(big, apw)
    small = []
    for base in (0, 4):
        x = setup(c, device, kernels, scale, actor_base=base, n=4)
        if big.eps is not None:
            x.eps = big.eps[:, base:base + 4].contiguous()
        if big.sig is not None:
            x.sig = big.sig[base:base + 4].contiguous()
        else:                                       # (PPO's per-actor noise scales are the agent's: its share of them)
            x.agent.batch_noise = lambda n, s=big.agent.batch_noise(8)[base:base + 4].contiguous(): s
        small.append((x, run(x, apw)[0]))
    return (big, gb, rows), small


def whole_steps(device, kernels=None, task='reach', J=2, n=5, scale=SCALE, layernorm=False, param_noise=None, apw=0,
                calls=CALLS):
    """DDPG with n_step 1 on the disturbed stream: every step closes, a row is (s, a, r, s') of one step -- n host chains
    over SyntheticEnv(task=, resets=, disturbance=) on the recorded actions give every row, the state left and the episode
    returns.  layernorm / param_noise ('normal': populations of 4 actors, n a multiple of 4): the actor variants of the
    launch.  -> (the monitor's returns, the chains')"""
    from surreal_amd import kernels as KN
    from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    prev = KN.set_default_kernels(kernels, device) if kernels is not None else None
    seed = SEEDS[task]
    try:
        D, A, S = obs_dim(task, J), J, sum(calls)
        lc, ec, sc = DC.configs(D, A, n, hidden=(8, 4), n_step=1, noise_type='normal', memory_size=n * S,
                                layernorm=layernorm, param_noise_type=param_noise)
        agent = DC.make_agent(lc, ec, sc)
        kw = dict(kernels=kernels) if kernels is not None else {}
        venv = SyntheticVecEnv(n, D, A, episode_len=EP, device=device, task=task, **kw)
        mon = venv.attach_monitor(capacity=4)
        venv.attach_resets(seed, 3, disturbance=scale)
        venv.reset()
        if param_noise:
            venv.attach_param_noise(agent, RC.SEED, actors_per_agent=4)
        replay = UniformReplay(lc, ec, sc)
        eps = torch.randn(S, n, A, generator=torch.Generator().manual_seed(5)).to(device)
        s0 = 0
        for T in calls:
            venv.ddpg_rollout_into(agent, replay, T, eps=eps[s0:s0 + T], actors_per_workgroup=apw)
            s0 += T
        f = {k: v.numpy() for k, v in EC.ring_fields(replay, ('obs', 'obs_next', 'actions', 'rewards', 'dones')).items()}
        state = venv.state.detach().cpu().numpy()
        got = AC.monitor_returns(mon, n)
    finally:
        if prev is not None:
            KN.set_default_kernels(*prev)
    flat = lambda o: o['low_dim']['flat_inputs']  # noqa: E731
    returns = []
    for a in range(n):
        h = SyntheticEnv(D, A, episode_len=EP, task=task, resets=(seed, 3 + a), disturbance=scale)
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


def per_step_chains(device, kernels=None, task='reach', J=2, n=70, scale=SCALE, steps=7, L_=3, base=None):
    """the per-step launch (SyntheticVecEnv.step) on a disturbed stream against n host envs: every state, the monitor's
    returns and its open sums; n = 70: one thread per actor, more than one wavefront"""
    from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv
    D, seed = obs_dim(task, J), SEEDS[task]
    base = 2 ** 32 - n if base is None else base
    kw = dict(kernels=kernels) if kernels is not None else {}
    venv = SyntheticVecEnv(n, D, J, episode_len=L_, device=device, task=task, **kw)
    mon = venv.attach_monitor(capacity=4)
    rs = venv.attach_resets(seed, actor_base=base, disturbance=scale)
    assert torch.equal(venv.reset(), rs.states(0)) and rs.episode == 1
    hosts = [SyntheticEnv(D, J, episode_len=L_, task=task, resets=(seed, base + a), disturbance=scale) for a in range(n)]
    for h in hosts:
        h._reset()
    returns = [[0.0] for _ in range(n)]
    acts = torch.randn(steps, n, J, generator=torch.Generator().manual_seed(4)) * 1.5
    for s in range(steps):
        state = venv.step(acts[s].to(device)).cpu()
        for a, h in enumerate(hosts):
            obs, r, done, _ = h._step(acts[s, a].numpy())
            returns[a][-1] += r
            if done:
                obs, _ = h._reset()
                returns[a].append(0.0)
            assert bits(state[a].numpy(), obs['low_dim']['flat_inputs']), (s, a)
    assert rs.episode == 1 + steps // L_
    assert AC.monitor_returns(mon, n) == [r[:steps // L_] for r in returns]
    assert mon.ep_reward.cpu().tolist() == [r[steps // L_] for r in returns]
    return venv


# ---- evaluation --------------------------------------------------------------------------------------------------------------

def host_eval_returns(task, J, n, E, L, action, resets, scale):
    """np.float64 [n, E]: the returns of E disturbed episodes of L steps per actor under the constant action `action`;
    resets = (seed, first_episode, actor_base): the fp64 step-order sum of the host step's fp32 rewards"""
    out = np.zeros((n, E), dtype=np.float64)
    act = np.full(J, action, dtype=np.float32)
    for a in range(n):
        for i in range(E):
            g, e = resets[2] + a, resets[1] + i
            s = TK.RESET_STATE[task](resets[0], g, e, J)
            total = 0.0
            for t in range(L):
                s, r = TK.STEP[task](s, act, w=TK.disturbance(resets[0], g, e, t, J), scale=scale)
                total = total + float(r)
            out[a, i] = total
    return out


def recorded_returns(p, n, E, L, agent, cfg, device, resets, scale):
    """device_eval_cases.recorded_returns on a disturbed stream: per episode a fresh env with a monitor, the stream
    attached with the scale and episode = first_episode + i, reset(), ONE episode through the recording launch"""
    import device_eval_cases as EV
    out = np.zeros((n, E), dtype=np.float64)
    for i in range(E):
        venv = EV.make_env(p, n, L, device)
        mon = venv.attach_monitor(capacity=2)
        rs = venv.attach_resets(resets[0], resets[2], disturbance=scale)
        rs.episode = resets[1] + i
        venv.reset()
        EV._rollout(p, venv, agent, EV._replay_of(p, cfg), L)
        counts, rewards, steps = EV._ring(mon)
        assert counts.tolist() == [1] * n and steps[:, 0].tolist() == [L] * n
        out[:, i] = rewards[:, 0]
    return out


# ---- the float64 restatements ------------------------------------------------------------------------------------------------

class _Disturbed(object):
    """mixin of a drawn-episode restatement env: the draws of (seed, actors, the episode under way, the step) and the
    scale, in float64 -- the draws are inputs (multiples of 2^-23: exact), the scale the fp32 value upcast"""

    def disturb(self, seed, g, scale, first_episode=0):
        self._dseed, self._dg, self._dscale = seed, np.asarray(g), float(np.float32(scale))
        self._depisode = first_episode

    def term(self):
        w = TK.disturbance(self._dseed, self._dg, self._depisode, self.t, self.A)
        return self._dscale * R.f64(torch.as_tensor(w))


class DisturbedReachEnv(_Disturbed, RR.DrawnReachEnv):
    def step(self, actions):
        J = self.A
        a = torch.clamp(actions, -1.0, 1.0)
        s = self.state
        p, v, g = s[:, :J], s[:, J:2 * J], s[:, 2 * J:]
        vr = (RC.C_VDECAY * v + RC.C_VGAIN * a) + self.term()
        vn = torch.clamp(vr, -1.0, 1.0)
        pr = p + RC.C_DT * vn
        pn = torch.clamp(pr, -10.0, 10.0)
        self.clip_margin = min(self.clip_margin, float((vr.abs() - 1.0).abs().min()), float((pr.abs() - 10.0).abs().min()))
        d = pn - g
        rew = -((d * d).sum(1) + RC.C_COST * (a * a).sum(1))
        return self._advance(s, torch.cat([pn, vn, g], 1), rew)

    def _advance(self, s, sn, rew):
        done = self.t + 1 >= self.L
        self.ep_sum, self.ep_abs, self.ep_len = self.ep_sum + rew, self.ep_abs + rew.abs(), self.ep_len + 1
        if done:
            self.finished.append((self.ep_sum, self.ep_abs, self.ep_len))
            self.ep_sum, self.ep_abs, self.ep_len = torch.zeros_like(rew), torch.zeros_like(rew), 0
            self.state = self.rows[self.begun].clone()
            self.begun += 1
            self._depisode += 1
        else:
            self.state = sn
        self.t = 0 if done else self.t + 1
        return s, sn, rew, done


class DisturbedArmEnv(_Disturbed, AC.ArmEnv):
    """arm_cases.ArmEnv whose i-th episode begins with rows[i] (float64 of the drawn fp32: exact), disturbed"""

    def __init__(self, rows, A, episode_len):
        self.rows = R.f64(torch.as_tensor(rows))
        super().__init__(self.rows[0], A, episode_len)
        self.begun = 1

    _advance = DisturbedReachEnv._advance

    def step(self, actions):
        J = self.A
        a = torch.clamp(actions, -1.0, 1.0)
        s = self.state
        th, om, g = s[:, :J], s[:, J:2 * J], s[:, 2 * J:]
        orr = (AC.C_WDECAY * om + AC.C_WGAIN * a) + self.term()
        on = torch.clamp(orr, -1.0, 1.0)
        tr = th + AC.C_DT * on
        tn = torch.clamp(tr, -AC.PI_F, AC.PI_F)
        self.clip_margin = min(self.clip_margin, float((orr.abs() - 1.0).abs().min()), float((tr.abs() - AC.PI_F).abs().min()))
        x2 = tn * tn
        sn_, cs_ = tn * AC.poly(x2, AC.SIN_C), AC.poly(x2, AC.COS_C)
        w = AC.link(J)
        dx, dy = cs_.sum(1) * w - g[:, 0], sn_.sum(1) * w - g[:, 1]
        rew = -((dx * dx + dy * dy) + AC.C_COST * (a * a).sum(1))
        return self._advance(s, torch.cat([tn, on, g], 1), rew)


def restatement(x, scale=SCALE):
    """reach_cases.restatement's on the disturbed drawn episodes -> (want {field: float64}, rows, written mask, the policy:
    .margins, .env)"""
    c, seed = x.c, SEEDS[x.task]
    g = x.base + np.arange(c.n)
    episodes = 1 + sum(CALLS) // EP
    rows = np.stack([TK.RESET_STATE[x.task](seed, g, e, c.A) for e in range(episodes + 1)])
    env = (DisturbedReachEnv if x.task == 'reach' else DisturbedArmEnv)(rows, c.A, EP)
    env.disturb(seed, g, scale)
    eps = R.f64(x.eps_ref)
    S = sum(CALLS)
    if c.family == 'ddpg':
        m = x.agent.model
        pol = RC.ProbedDdpgPolicy({k: v for k, v in m.actor.views.items()}, c.n, c.A, noise='ou_noise', sigmas=x.sig,
                                  theta=x.agent.theta, dt=x.agent.dt)
        pol.margins = RC.Margins()
        ring, nrows, written = R.ddpg_ring(pol, env, eps, S, N_STEP, GAMMA, x.capacity)
    else:
        p, zf, lstm, ns = EC.ppo_reference_inputs(x.agent, c.n)
        pol = RC.ProbedPpoPolicy(p, zf, lstm, ns)
        pol.margins = RC.Margins()
        ring, nrows, written = R.ppo_windows(pol, env, eps, S, N_STEP, STRIDE, x.capacity)
    pol.env = env
    return ring, nrows, written, pol


# per case: the first seed of the agent's parameters under which the restatement ALONE keeps every ReLU pre-activation,
# action clip and environment clamp MARGIN from its kink at SCALE (python tests/task_disturbance_cases.py prints them)
RESTATED = ['reach-window-J5', 'reach-lstm_window-J2', 'reach-ddpg-J21', 'arm-window-J30', 'arm-lstm_window-J5', 'arm-ddpg-J5']
TUNED = {
    'reach-window-J5': 0,
    'reach-lstm_window-J2': 3,
    'reach-ddpg-J21': 0,
    'arm-window-J30': 8,
    'arm-lstm_window-J5': 11,
    'arm-ddpg-J5': 6,
}


def tune(c, seeds=range(1, 200)):
    for seed in [c.base.seed] + list(seeds):
        x = setup(c, 'cpu', DisturbedCpuKernels(), seed=seed)
        try:
            RC.input_conditions(restatement(x)[3], RC.MARGIN)
            return seed
        except AssertionError:
            continue
    return None


if __name__ == '__main__':          # prints TUNED's entries
    from surreal_amd import kernels as _KN
    _KN.set_default_kernels(DisturbedCpuKernels(), 'cpu')
    for cid in RESTATED:
        print('    %r: %r,' % (cid, tune(BY_ID[cid])), flush=True)
