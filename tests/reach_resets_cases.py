"""
`reach` with its episodes drawn from a reset stream (SyntheticVecEnv.attach_resets; surreal_amd/env/tasks.py
reach_reset_state), shared by the CPU tier (test_reach_resets_cpu.py) and the GPU tier (test_gpu_reach_resets.py).  The
shapes, calls and bounds are reach_cases' own; what changes is where an episode begins:

  * ``DrawnReachEnv``  -- reach_cases.ReachEnv (float64) restarting from the drawn rows, upcast (exact);
  * ``setup`` / ``run`` / ``restatement`` -- reach_cases' with the stream attached and the env reset onto episode 0;
  * ``host_episodes``  -- n host chains over ``SyntheticEnv(task='reach', resets=(seed, g))`` driven with recorded actions;
  * ``tuned``          -- (seed, scale) per case, found on the CPU on the float64 restatement alone
    (``python tests/reach_resets_cases.py`` prints the pairs that differ from the case's own).
"""
import numpy as np
import torch

import reach_cases as RC
import rollout_envelope_cases as EC
import rollout_fp64_ref as R
from surreal_amd.env import tasks as TK

RSEED = 0xC2B2AE3D27D4EB4F            # the reset stream's seed (the noise stream's is reach_cases.SEED)
EPISODES = 3                          # T = 12 over episodes of 5: episodes 0 and 1 end inside, 2 is open at the end

CASES = RC.CASES
# (seed, scale): the first the float64 restatement alone meets the input conditions with, on drawn episodes
TUNED = {
    'window-63-21-n20': (1, 3.0),
    'lstm_window-6-2-n5-streams': (2, 3.0),
    'lstm_window-63-21-n20': (3, 3.0),
    'ddpg-63-21-n20-streams': (2, 6.0),
}


def tuned(c):
    seed, scale = TUNED.get(c.id, (c.seed, c.scale))
    return c._replace(seed=seed, scale=scale)


def rows_of(n, J, actor_base=0, episodes=EPISODES, first=0, seed=RSEED):
    """np [episodes, n, 3 J] fp32: the rows the actors actor_base .. actor_base + n - 1 begin episodes first .. with"""
    g = actor_base + np.arange(n)
    return np.stack([TK.reach_reset_state(seed, g, first + e, J) for e in range(episodes)])


class DrawnReachEnv(RC.ReachEnv):
    """ReachEnv whose i-th episode begins with rows[i] (float64 of the drawn fp32: exact)"""

    def __init__(self, rows, A, episode_len):
        self.rows = R.f64(torch.as_tensor(rows))
        super().__init__(self.rows[0], A, episode_len)
        self.begun = 1

    def step(self, actions):
        s, sn, rew, done = super().step(actions)
        if done:
            self.state = self.rows[self.begun].clone()
            self.begun += 1
        return s, sn, rew, done


def setup(c, device, kernels=None, wrap=True, actor_base=0, attach=True):
    """reach_cases.setup, then the reset stream attached and episode 0 begun (attach=False: the stream is made and handed
    back in x.resets but not attached -- the caller wants it disabled)"""
    x = RC.setup(c, device, kernels, wrap=wrap)
    if actor_base and x.venv.noise is not None:
        x.venv.attach_noise(RC.SEED, actor_base)
        x.eps_ref = x.venv.noise.draws(sum(RC.CALLS))
    x.resets = x.venv.attach_resets(RSEED, actor_base)
    if attach:
        x.venv.reset()
    else:
        x.venv.detach_resets()
    return x


def run(x, apw=0, calls=RC.CALLS):
    """reach_cases.run over `calls`"""
    prev, RC.CALLS = RC.CALLS, calls
    try:
        return RC.run(x, apw)
    finally:
        RC.CALLS = prev


def restatement(x, actor_base=0):
    """reach_cases.restatement on DrawnReachEnv"""
    c = x.c
    env = DrawnReachEnv(rows_of(c.n, c.A, actor_base), c.A, RC.EP)
    eps = R.f64(x.eps_ref)
    S = sum(RC.CALLS)
    if c.family == 'ddpg':
        m = x.agent.model
        pol = RC.ProbedDdpgPolicy({k: v for k, v in m.actor.views.items()}, c.n, c.A, noise='ou_noise', sigmas=x.sig,
                                  theta=x.agent.theta, dt=x.agent.dt)
        pol.margins = RC.Margins()
        ring, rows, written = R.ddpg_ring(pol, env, eps, S, RC.N_STEP, RC.GAMMA, x.capacity)
    else:
        p, zf, lstm, ns = EC.ppo_reference_inputs(x.agent, c.n)
        pol = RC.ProbedPpoPolicy(p, zf, lstm, ns)
        pol.margins = RC.Margins()
        ring, rows, written = R.ppo_windows(pol, env, eps, S, RC.N_STEP, RC.STRIDE, x.capacity)
    pol.env = env
    return ring, rows, written, pol


def host_env(c, g, episode_len=RC.EP, seed=RSEED):
    from surreal_amd.env.synthetic_env import SyntheticEnv
    return SyntheticEnv(c.D, c.A, episode_len=episode_len, task='reach', resets=(seed, g))


def tune(c, seeds=range(60)):
    """reach_cases.tune on the drawn episodes"""
    from reach_resets_cpu_kernels import ResetsCpuKernels
    for seed in [c.seed] + list(seeds):
        t = c._replace(seed=seed)
        x = setup(t, 'cpu', ResetsCpuKernels(), wrap=False)
        try:
            RC.input_conditions(restatement(x)[3], (2 if c.streams else 1) * RC.MARGIN)
            return seed, c.scale
        except AssertionError:
            continue
    return None


if __name__ == '__main__':          # prints TUNED's entries
    from reach_resets_cpu_kernels import ResetsCpuKernels as _K
    from surreal_amd import kernels as _KN
    _KN.set_default_kernels(_K(), 'cpu')
    for c_ in CASES:
        got_ = tune(c_)
        if got_ != (c_.seed, c_.scale):
            print('    %r: %r,' % (c_.id, got_), flush=True)


# ---- the checks both tiers run (the CPU tier on the double, the GPU tier on the kernels) -----------------------------------

def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def flat(obs):
    return obs['low_dim']['flat_inputs']


def window_chains(got, x, actor_base=0):
    """a windowed case's ring (rows to spare, calls of reach_cases.CALLS from episode 0) against n host chains over
    SyntheticEnv(task='reach', resets=(RSEED, g)): windows of 3 steps, 2 apart, cover every step of an episode of 5, so
    the recorded actions drive the chain through episodes 0 and 1, the carry's through the two steps of episode 2; every
    observation, reward, done, the state left and (-> returned, [n][2]) the episode returns"""
    c, n, N = x.c, x.c.n, RC.N_STEP
    assert (RC.EP, N, RC.STRIDE, sum(RC.CALLS)) == (5, 3, 2, 12)
    f = {k: got[k].numpy() for k in ('obs', 'obs_next', 'actions', 'rewards', 'dones')}
    carry = x.venv._ppo['carry']['actions'].detach().cpu().numpy()
    returns = []
    for a in range(n):
        h = host_env(c, actor_base + a)
        returns.append([])
        for e in range(2):
            rows = [(2 * e + w) * n + a for w in range(2)]
            obs = np.concatenate([f['obs'][rows[0]].reshape(N, c.D), f['obs'][rows[1]].reshape(N, c.D)[1:]])
            act = np.concatenate([f['actions'][rows[0]].reshape(N, c.A), f['actions'][rows[1]].reshape(N, c.A)[1:]])
            rew = np.concatenate([f['rewards'][rows[0]].reshape(N), f['rewards'][rows[1]].reshape(N)[1:]])
            assert bits(f['obs'][rows[1]].reshape(N, c.D)[0], obs[2])           # (step 2 is in both windows)
            o, _ = h._reset()
            total = 0.0
            for u in range(RC.EP):
                assert bits(flat(o), obs[u]), (a, e, u)
                o, r, done, _ = h._step(act[u])
                assert bits(np.float32(r), rew[u]), (a, e, u)
                total += r
                if u == 2:
                    assert bits(flat(o), f['obs_next'][rows[0]])
            assert done and bits(flat(o), f['obs_next'][rows[1]])
            assert f['dones'][rows[0]].tolist() == [0.0] * N and f['dones'][rows[1]].tolist() == [0.0] * (N - 1) + [1.0]
            returns[-1].append(total)
        o, _ = h._reset()
        for u in range(2):
            o, _, _, _ = h._step(carry[a, u])
        assert bits(flat(o), got['state'][a].numpy()), a
    return returns


def ddpg_chains(got, x, actor_base=0):
    """a DDPG case's ring likewise: transition j = 0, 1, 2 of an episode of 5 holds (s_j, a_j) and the state after step
    j + 2, so from each episode's drawn row the chain follows s_0 .. s_3 on recorded actions"""
    c, n, N = x.c, x.c.n, RC.N_STEP
    f = {k: got[k].numpy() for k in ('obs', 'obs_next', 'actions', 'dones')}
    for a in range(n):
        h = host_env(c, actor_base + a)
        for e in range(2):
            rows = [(3 * e + j) * n + a for j in range(3)]
            o, _ = h._reset()
            for j in range(3):
                assert bits(flat(o), f['obs'][rows[j]]), (a, e, j)
                o, _, _, _ = h._step(f['actions'][rows[j]])
            assert bits(flat(o), f['obs_next'][rows[0]]), (a, e)
            assert [float(f['dones'][r].reshape(-1)[0]) for r in rows] == [0.0, 0.0, 1.0]


def ddpg_whole_steps(device, kernels=None, n=5, J=2, monitor=True):
    """n_step 1: every step closes, a row is (s, a, r, s') of one step -- so n host chains on the recorded actions give
    every row, the state left and the monitor's episode returns.  -> (polled [(actor, return, steps)], the chains'
    returns [n][2])"""
    from surreal_amd import kernels as KN
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    import ddpg_rollout_cases as DC
    prev = KN.set_default_kernels(kernels, device) if kernels is not None else None
    try:
        D, A, S = 3 * J, J, sum(RC.CALLS)
        lc, ec, sc = DC.configs(D, A, n, hidden=(8, 4), n_step=1, noise_type='normal', memory_size=n * S)
        agent = DC.make_agent(lc, ec, sc)
        kw = dict(kernels=kernels) if kernels is not None else {}
        venv = SyntheticVecEnv(n, D, A, episode_len=RC.EP, device=device, task='reach', **kw)
        mon = venv.attach_monitor(capacity=4)
        venv.attach_resets(RSEED, 3)
        venv.reset()
        replay = UniformReplay(lc, ec, sc)
        eps = torch.randn(S, n, A, generator=torch.Generator().manual_seed(5)).to(device)
        s0 = 0
        for T in RC.CALLS:
            venv.ddpg_rollout_into(agent, replay, T, eps=eps[s0:s0 + T])
            s0 += T
        f = {k: v.numpy() for k, v in EC.ring_fields(replay, ('obs', 'obs_next', 'actions', 'rewards', 'dones')).items()}
        state = venv.state.detach().cpu().numpy()
        polled = mon.poll()
    finally:
        if prev is not None:
            KN.set_default_kernels(*prev)
    c = RC.Case('whole', 'ddpg', D, A, n, None, 0, 1.0, False)
    returns = []
    for a in range(n):
        h = host_env(c, 3 + a)
        o, _ = h._reset()
        returns.append([0.0])
        for s in range(S):
            row = s * n + a
            assert bits(flat(o), f['obs'][row]), (a, s)
            o, r, done, _ = h._step(f['actions'][row])
            assert bits(flat(o), f['obs_next'][row]) and bits(np.float32(r), f['rewards'][row].reshape(-1)[0]), (a, s)
            assert float(f['dones'][row].reshape(-1)[0]) == float(done)
            returns[-1][-1] += r
            if done:
                o, _ = h._reset()
                returns[-1].append(0.0)
        assert bits(flat(o), state[a])
    return polled, [r[:2] for r in returns]


def rounded(returns):
    """host chains' episode returns as a monitor reports them (EpisodeMonitor's and poll()'s round(., 6))"""
    return [[round(r, 6) for r in per_actor] for per_actor in returns]


def polled_returns(polled, n):
    out = [[] for _ in range(n)]
    for a, reward, steps in polled:
        assert steps == RC.EP
        out[a].append(reward)
    return out


def split_envs(c, device, kernels=None, apw=0):
    """-> (one env of 8 actors, its ring; [two envs of 4 actors, actor_base 0 and 4, and their rings]): the case's
    agent at n = 8 and n = 4 has the same parameters; an env without a noise stream gets its share of the draws"""
    big = setup(c._replace(n=8), device, kernels, wrap=False)
    gb, _ = run(big, apw)
    small = []
    for base in (0, 4):
        x = setup(c._replace(n=4), device, kernels, wrap=False, actor_base=base)
        if big.eps is not None:
            x.eps = big.eps[:, base:base + 4].contiguous()
        if big.sig is not None:
            x.sig = big.sig[base:base + 4].contiguous()
        else:                                       # (PPO's per-actor noise scales are the agent's: its share of them)
            x.agent.batch_noise = lambda n, s=big.agent.batch_noise(8)[base:base + 4].contiguous(): s
        small.append((x, run(x, apw)[0]))
    return (big, gb), small


def same_actors(gb, small, rows):
    """every field of the 8-actor ring holds, actor by actor, the two 4-actor rings' bytes"""
    for k, v in gb.items():
        if k in ('state', 'ou', 'hN', 'cN'):
            parts = torch.cat([g[k] for _, g in small])
            assert torch.equal(v.contiguous().view(torch.uint8), parts.contiguous().view(torch.uint8)), k
            continue
        steps = rows // 8
        whole = v[:rows].reshape(steps, 8, -1)
        parts = torch.cat([g[k][:rows // 2].reshape(steps, 4, -1) for _, g in small], 1)
        assert torch.equal(whole.contiguous().view(torch.uint8), parts.contiguous().view(torch.uint8)), k
