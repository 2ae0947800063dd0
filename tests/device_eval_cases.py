"""
Evaluation on the device (SyntheticVecEnv.evaluate; smx_synth_ppo_eval_f32 / smx_synth_ddpg_eval_f32), shared by the CPU
tier (test_device_eval_cpu.py) and the GPU tier (test_gpu_device_eval.py):

  * the shapes: (n, E, L) with 15 rows (a tail at every block size), 1 row and 18 rows (two blocks at 16 rows per
    workgroup); the policies -- plain MLP, LSTM stem of 10 units (padded to 12), plain DDPG actor -- on `reach` with 1, 2
    and 21 masses and on `drift` with (D, A) = (17, 6);
  * ``host_returns`` -- the host definition of an evaluation under a CONSTANT action: the fp64 step-order sum of the fp32
    step rewards of tasks.reach_step from tasks.reach_reset_state (or init_state), of the host SyntheticEnv on drift.  It
    calls no device policy code;
  * ``recorded_returns`` -- the recording launches' answer, row by row: a fresh env with a monitor per (actor, episode),
    one episode through ppo_rollout_into / ddpg_rollout_into, the monitor's finished-episode ring read raw (fp64).
"""
import collections

import numpy as np
import torch

import ddpg_rollout_cases as DC
import ppo_window_cases as PW
from surreal_amd.env import tasks as TK

SHAPES = [(5, 3, 7), (1, 1, 1), (9, 2, 4)]                 # (n, E, L): 15 rows, 1 row, 18 rows
BLOCKS = (4, 8, 16)
RSEED = 0xC2B2AE3D27D4EB4F                                 # the reset stream's seed
NSEED = 0x9E3779B97F4A7C15                                 # the noise stream's
FIRST_EPISODES = (0, 2 ** 32 - 2)                          # with E = 3 the low counter word carries inside the call
FIRST_STEP = 2 ** 32 - 5                                   # the draw step's low word carries inside an episode of 7
RNN = 10                                                   # logical LSTM units (padded to 12)

Policy = collections.namedtuple('Policy', 'id family task D A hidden')
POLICIES = [
    Policy('mlp-reach-J2', 'mlp', 'reach', 6, 2, (32, 32)),
    Policy('mlp-reach-J1', 'mlp', 'reach', 3, 1, (32, 32)),
    Policy('mlp-reach-J21', 'mlp', 'reach', 63, 21, (32, 32)),
    Policy('mlp-drift-17-6', 'mlp', 'drift', 17, 6, (32, 32)),
    Policy('lstm-reach-J2', 'lstm', 'reach', 6, 2, (32, 32)),
    Policy('lstm-reach-J21', 'lstm', 'reach', 63, 21, (32, 32)),
    Policy('lstm-drift-17-6', 'lstm', 'drift', 17, 6, (32, 32)),
    Policy('ddpg-reach-J2', 'ddpg', 'reach', 6, 2, (32, 32)),
    Policy('ddpg-reach-J1', 'ddpg', 'reach', 3, 1, (32, 32)),
    Policy('ddpg-reach-J21', 'ddpg', 'reach', 63, 21, (32, 32)),
    Policy('ddpg-drift-17-6', 'ddpg', 'drift', 17, 6, (32, 32)),
]
# the most ragged hidden pair smx_synth_eval_supported accepts: multiples of 4 that are no multiple of 8, 16 or 32 --
# partial feature tiles and a partial K chunk in every layer (test_device_eval_cpu.py checks the neighbours are refused)
RAGGED = (28, 20)
POLICIES += [Policy('mlp-reach-J2-ragged', 'mlp', 'reach', 6, 2, RAGGED),
             Policy('lstm-reach-J2-ragged', 'lstm', 'reach', 6, 2, RAGGED),
             Policy('ddpg-reach-J2-ragged', 'ddpg', 'reach', 6, 2, RAGGED)]
# the smallest H2 past the split output layer (pack_chunks(260) = 10 chunks > 8 waves): the recording and the evaluation
# kernels both take the generic output-layer loop (rollout_envelope_cases.py's wide-24-260 pair)
WIDE = (24, 260)
POLICIES += [Policy('mlp-reach-J2-wide', 'mlp', 'reach', 6, 2, WIDE),
             Policy('lstm-reach-J2-wide', 'lstm', 'reach', 6, 2, WIDE)]
BY_ID = {p.id: p for p in POLICIES}


def actor_bases(n):
    return (0, 2 ** 32 - n)


def same_f64(a, b):
    """two fp64 arrays hold the same bits"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- agents ----------------------------------------------------------------------------------------------------------------

def ppo_agent(p, mode='eval_deterministic_local', seed=3, n_step=1, stride=1, memory_size=4096):
    """a PPO agent of policy p in an evaluation mode: z-filter with non-trivial running sums, a last layer that reaches
    the clip (windows of one step: an episode of any length closes some)"""
    from surreal_amd import synthetic
    from surreal_amd.agent import PPOAgent
    rnn = RNN if p.family == 'lstm' else None
    lc, ec, sc = PW.configs(p.D, p.A, n_step, stride, p.hidden, rnn, True, memory_size)
    agent = PPOAgent(lc, ec, sc, agent_id=1, agent_mode=mode)
    agent.model.load_params(synthetic.make_ppo_params(p.D, p.A, hidden=tuple(p.hidden), seed=seed, final_scale=2.0,
                                                      log_sig_spread=0.4, rnn_hidden=rnn or 0))
    agent.model.z_filter.load_state_dict(synthetic.make_zfilter_state(p.D, seed=seed + 1))
    return agent, (lc, ec, sc)


def ddpg_agent(p, n, mode='eval_deterministic_local', seed=3, n_step=1, memory_size=4096, layernorm=False,
               param_noise_type=None):
    lc, ec, sc = DC.configs(p.D, p.A, n, hidden=p.hidden, n_step=n_step, memory_size=memory_size, layernorm=layernorm,
                            param_noise_type=param_noise_type, folder='surreal_amd_device_eval')
    agent = DC.make_agent(lc, ec, sc, mode=mode, seed=seed, w3_scale=1.0)
    # the actor's parameters from numpy (torch's initialisation depends on the device): uniform in +-1 / sqrt(fan_in), the
    # output layer's weights times 6 so that actions reach the clip
    rs = np.random.RandomState(1000 + seed)
    with torch.no_grad():
        for i, fan_in in ((1, p.D), (2, p.hidden[0]), (3, p.hidden[1])):
            for k in ('W%d' % i, 'b%d' % i):
                v = agent.model.actor.views[k]
                w = rs.uniform(-1.0, 1.0, size=tuple(v.shape)).astype(np.float32) / np.float32(np.sqrt(fan_in))
                v.copy_(torch.as_tensor(w * np.float32(6.0 if k == 'W3' else 1.0)))
    return agent, (lc, ec, sc)


def make_agent(p, n, mode='eval_deterministic_local', **kw):
    return ddpg_agent(p, n, mode, **kw) if p.family == 'ddpg' else ppo_agent(p, mode, **kw)


def constant_policy(agent, value=0.0):
    """every weight of the actor zero, the output bias `value`: the output layer's sum is exactly `value` whatever the
    observation (an LSTM stem in front changes nothing: its output meets zero weights)"""
    with torch.no_grad():
        for k, v in agent.model.actor.views.items():
            v.zero_()
        agent.model.actor.views['b3'].fill_(float(value))


def make_env(p, n, L, device, kernels=None, **kw):
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    if kernels is not None:
        kw['kernels'] = kernels
    return SyntheticVecEnv(n, p.D, p.A, episode_len=L, seeds=list(range(n)), device=device, task=p.task, **kw)


# ---- the host definition under a constant action -----------------------------------------------------------------------------

def host_returns(p, n, E, L, action, resets=None, init_state=None):
    """np.float64 [n, E]: the returns of E episodes of L steps per actor under the constant action `action` (a float; the
    environment clips it).  resets = (seed, first_episode, actor_base): episode i of actor a begins with
    tasks.reach_reset_state(seed, actor_base + a, first_episode + i, J); None: with init_state[a] (np [n, D]).  reach: the
    fp64 sum, in step order, of tasks.reach_step's fp32 rewards; drift: the host SyntheticEnv's episode"""
    out = np.zeros((n, E), dtype=np.float64)
    act = np.full(p.A, action, dtype=np.float32)
    for a in range(n):
        for i in range(E):
            if p.task == 'reach':
                if resets is not None:
                    s = TK.reach_reset_state(resets[0], resets[2] + a, resets[1] + i, p.A)
                else:
                    s = np.asarray(init_state[a], dtype=np.float32)
                total = 0.0
                for _ in range(L):
                    s, r = TK.reach_step(s, act)
                    assert np.asarray(r).dtype == np.float32
                    total = total + float(r)
                out[a, i] = total
            else:
                from surreal_amd.env.synthetic_env import SyntheticEnv
                env = SyntheticEnv(p.D, p.A, episode_len=L, seed=a)
                assert init_state is None or np.array_equal(env.init_state, np.asarray(init_state[a]))
                env._reset()
                total, done = 0.0, False
                while not done:
                    _, r, done, _ = env._step(act)
                    total = total + float(np.float32(r))
                out[a, i] = total
    return out


# ---- the recording launches, row by row ------------------------------------------------------------------------------------

def _replay_of(p, cfg):
    from surreal_amd.replay import FIFOReplay, UniformReplay
    return (UniformReplay if p.family == 'ddpg' else FIFOReplay)(*cfg)


def _rollout(p, venv, agent, replay, T, apw=0):
    if p.family == 'ddpg':
        venv.ddpg_rollout_into(agent, replay, T, actors_per_workgroup=apw)
    else:
        agent._batch_cells = None                       # (every episode from the zero state)
        venv.ppo_rollout_into(agent, replay, T, actors_per_workgroup=apw)


def _ring(mon):
    """the monitor's finished episodes raw: (counts [n], returns fp64 [n, capacity], steps [n, capacity])"""
    return mon.ep_count.cpu().numpy(), mon.done_reward.cpu().numpy(), mon.done_steps.cpu().numpy()


def recorded_returns(p, n, E, L, agent, cfg, device, resets=None, noise=None):
    """np.float64 [n, E]: for each episode i a fresh env with a monitor (the stream attached with episode =
    first_episode + i and reset(); the noise stream at step first_step + i L), ONE episode through the recording launch,
    the monitor's ring raw.  resets = (seed, first_episode, actor_base), noise = (seed, first_step, actor_base) or None"""
    out = np.zeros((n, E), dtype=np.float64)
    for i in range(E):
        venv = make_env(p, n, L, device)
        mon = venv.attach_monitor(capacity=2)
        if resets is not None:
            rs = venv.attach_resets(resets[0], resets[2])
            rs.episode = resets[1] + i
            venv.reset()
        if noise is not None:
            ns = venv.attach_noise(noise[0], noise[2])
            ns.step = noise[1] + i * L
        _rollout(p, venv, agent, _replay_of(p, cfg), L)
        counts, rewards, steps = _ring(mon)
        assert counts.tolist() == [1] * n and steps[:, 0].tolist() == [L] * n
        out[:, i] = rewards[:, 0]
    return out


def serial_returns(p, n, E, L, agent, cfg, device, resets=None, noise=None):
    """the same from ONE call of T = E L on one env with the streams attached: the E returns per actor in order"""
    venv = make_env(p, n, L, device)
    mon = venv.attach_monitor(capacity=E)
    if resets is not None:
        rs = venv.attach_resets(resets[0], resets[2])
        rs.episode = resets[1]
        venv.reset()
    if noise is not None:
        ns = venv.attach_noise(noise[0], noise[2])
        ns.step = noise[1]
    _rollout(p, venv, agent, _replay_of(p, cfg), E * L)
    counts, rewards, steps = _ring(mon)
    assert counts.tolist() == [E] * n and (steps == L).all()
    return rewards.copy()


# ---- DeviceEvaluator's reports against host EvalTensorplexMonitors ------------------------------------------------------------

class _ReplayedEpisodes(object):
    """a host env whose k-th episode is ONE step with reward returns[k] (an EpisodeMonitor around it reports
    round(returns[k], 6), steps 1)"""

    def __init__(self, returns):
        self.returns, self.k = list(returns), 0

    def reset(self):
        return None, {}

    def step(self, action):
        r = self.returns[self.k]
        self.k += 1
        return None, r, True, {}


def check_reports(de, per_actor, id_base, session_config, separate_plots=False):
    """de.reports[i] after its runs against EvalTensorplexMonitor(eval_id = id_base + i) around a host env fed
    per_actor[i] (every return of actor i, in order): the same name, and per report the same global_step, tags and
    'reward' scalar (step_per_s is wall time on both sides: present, not compared)"""
    from surreal_amd.env import EvalTensorplexMonitor
    assert len(de.reports) == len(per_actor)
    for i, returns in enumerate(per_actor):
        host = EvalTensorplexMonitor(_ReplayedEpisodes(returns), eval_id=id_base + i, fetch_parameter=lambda: None,
                                     session_config=session_config, separate_plots=separate_plots, sleep=lambda s: None)
        for _ in returns:
            host.reset()
            host.step(None)
        dev = de.reports[i]
        assert dev.tensorplex_name == host.tensorplex_name == 'eval/%d' % (id_base + i)
        assert dev.num_episodes == host.num_episodes == len(returns)
        assert dev.episode_rewards == host.episode_rewards
        h, d = host.tensorplex.history, dev.tensorplex.history
        period = session_config['tensorplex']['update_schedule']['eval_env']
        assert len(h) == len(d) == len(returns) // period
        for (hs, hv), (ds, dv) in zip(h, d):
            tag = ':reward' if separate_plots else 'reward'
            assert hs == ds and set(hv) == set(dv) == {tag, 'step_per_s'}
            assert hv[tag] == dv[tag]


# ---- the refusals ----------------------------------------------------------------------------------------------------------------

def check_python_refusals(device, kernels):
    """every refusal of SyntheticVecEnv.evaluate (the caller checks that nothing was launched); kernels: the kernels
    object of the envs (None: the default one)"""
    import types

    import pytest
    mlp, ddpg, drift = BY_ID['mlp-reach-J2'], BY_ID['ddpg-reach-J2'], BY_ID['mlp-drift-17-6']
    n, L = 5, 4
    env = lambda p, **kw: make_env(p, n, L, device, kernels, **kw)  # noqa: E731
    agent, _ = make_agent(mlp, n)
    dagent, _ = make_agent(ddpg, n)
    venv = env(mlp)
    assert venv.can_evaluate(agent) and venv.can_evaluate(dagent)

    def refused(cls, words, v, a, **kw):
        with pytest.raises(cls) as e:
            v.evaluate(a, **kw)
        assert type(e.value) is cls and all(w in str(e.value) for w in words), str(e.value)

    # NotImplementedError: what the launch does not run
    cam_env = env(drift, pixel=(3, 8, 8))
    refused(NotImplementedError, ('evaluate', 'a camera env', 'only'), cam_env, make_agent(drift, n)[0])
    cam_agent = types.SimpleNamespace(model=types.SimpleNamespace(if_pixel=True), rnn_config=agent.rnn_config,
                                      agent_mode='eval_deterministic_local')
    refused(NotImplementedError, ('a camera agent',), venv, cam_agent)
    assert not venv.can_evaluate(cam_agent) and not cam_env.can_evaluate(agent)
    clocks = make_env(drift, n, [L] * n, device, kernels)
    refused(NotImplementedError, ('per-actor episode clocks',), clocks, make_agent(drift, n)[0])
    ln, _ = ddpg_agent(ddpg, n, layernorm=True)
    refused(NotImplementedError, ('a LayerNorm actor',), venv, ln)
    noisy = env(ddpg)
    noisy.param_noise = object()
    refused(NotImplementedError, ('an attached parameter noise',), noisy, dagent)
    assert noisy.can_evaluate(agent)                                    # (a PPO policy has none)
    lstm, _ = make_agent(BY_ID['lstm-reach-J2'], n)
    lstm.rnn_config.rnn_layer = 2
    try:
        refused(NotImplementedError, ('rnn_layer 2',), venv, lstm)
    finally:
        lstm.rnn_config.rnn_layer = 1
    refused(NotImplementedError, ('DDPG', 'eval_stochastic'), venv, make_agent(ddpg, n, mode='eval_stochastic_local')[0],
            noise=(NSEED, 0))
    odd = make_agent(mlp._replace(hidden=(30, 32)), n)[0]
    refused(NotImplementedError, ('smx_synth_eval_supported',), venv, odd)
    assert not venv.can_evaluate(odd) and not venv.can_evaluate(ln)
    # ValueError: the mode, the streams, the sizes
    refused(ValueError, ('training',), venv, make_agent(mlp, n, mode='training')[0])
    refused(ValueError, ('no reset distribution',), env(drift), make_agent(drift, n)[0], resets=(RSEED, 0))
    refused(ValueError, ('noise must be None',), venv, agent, noise=(NSEED, 0))
    refused(ValueError, ('noise=', 'required'), venv, make_agent(mlp, n, mode='eval_stochastic_local')[0])
    refused(ValueError, ('episodes',), venv, agent, episodes=0)
    refused(ValueError, ('first_episode', 'negative'), venv, agent, resets=(RSEED, -1))
    refused(ValueError, ('2^32',), venv, agent, resets=(RSEED, 0, 2 ** 32 - n + 1))
    refused(ValueError, ('2^32',), venv, agent, resets=(RSEED, 0, -1))
    refused(ValueError, ('out',), venv, agent, out=torch.empty(n, 1, device=device))
    refused(ValueError, ('2^31',), venv, agent, episodes=2 ** 31 // n + 1)


E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3              # include/surreal_amd.h


def check_entry_point_codes():
    """the C entry points' argument checks, which run before any launch (host code: no GPU needed)"""
    from surreal_amd import _lib as L
    import ctypes
    lib = L.load()

    def net(D=6, H1=32, H2=32, A=2):
        m = L.Mlp3()
        m.W1 = m.b1 = m.W2 = m.b2 = m.W3 = m.b3 = 4096
        m.D, m.H1, m.H2, m.OUT = D, H1, H2, A
        return m

    def stream(cls, base=0, counter=0, enabled=1):
        q = cls()
        q.seed, q.actor_base, q.enabled = 1, base, enabled
        setattr(q, 'episode' if cls is L.ResetStream else 'step', counter)
        return q

    def ppo(task=1, n=4, episodes=2, episode_len=3, resets=None, noise=None, apw=0, m=None, **fields):
        m = m or net()
        p = L.SynthPpoEval()
        p.net, p.packed, p.log_var, p.init_state, p.returns = ctypes.pointer(m), 4096, 4096, 4096, 4096
        p.n, p.episodes, p.episode_len, p.task, p.actors_per_workgroup = n, episodes, episode_len, task, apw
        if resets is not None:
            p.resets = resets
        if noise is not None:
            p.noise = noise
        for k, v in fields.items():
            setattr(p, k, v)
        return lib.smx_synth_ppo_eval_f32(p, None)

    def ddpg(task=1, n=4, episodes=2, episode_len=3, resets=None, apw=0, m=None, **fields):
        m = m or net()
        p = L.SynthDdpgEval()
        p.net, p.packed, p.init_state, p.returns = ctypes.pointer(m), 4096, 4096, 4096
        p.n, p.episodes, p.episode_len, p.task, p.actors_per_workgroup = n, episodes, episode_len, task, apw
        if resets is not None:
            p.resets = resets
        for k, v in fields.items():
            setattr(p, k, v)
        return lib.smx_synth_ddpg_eval_f32(p, None)
    R, N = L.ResetStream, L.NoiseStream
    for f in (ppo, ddpg):
        # an enabled reset stream on drift; what smx_synth_task_supported refuses
        assert f(task=0, m=net(D=17, A=6), resets=stream(R)) == E_UNSUPPORTED
        assert f(task=1, m=net(D=7, A=2)) == E_UNSUPPORTED and f(task=1, m=net(D=66, A=22)) == E_UNSUPPORTED
        assert f(task=7) == E_UNSUPPORTED
        assert f(m=net(H1=30)) == E_UNSUPPORTED                         # (a shape the kernels do not take)
        # the stream's ids and index, the sizes
        assert f(resets=stream(R, base=-1)) == E_SHAPE and f(resets=stream(R, base=2 ** 32 - 3)) == E_SHAPE
        assert f(resets=stream(R, counter=-1)) == E_SHAPE
        assert f(episodes=0) == E_SHAPE and f(episode_len=0) == E_SHAPE and f(n=0) == E_SHAPE
        assert f(n=2 ** 20, episodes=2 ** 11) == E_SHAPE                # (n * episodes = 2^31)
        assert f(apw=5) == E_SHAPE
        # required pointers
        for k in ('net', 'packed', 'init_state', 'returns'):
            assert f(**{k: None}) == E_NULL, k
    assert lib.smx_synth_ppo_eval_f32(None, None) == E_NULL and lib.smx_synth_ddpg_eval_f32(None, None) == E_NULL
    assert ppo(log_var=None) == E_NULL
    assert ppo(noise=stream(N, base=-1)) == E_SHAPE and ppo(noise=stream(N, base=2 ** 32 - 3)) == E_SHAPE
    assert ppo(zsum=4096) == E_NULL and ppo(zsum=4096, zsumsq=4096) == E_NULL       # the z-filter's three: all or none
    assert ppo(resets=stream(R, base=-1, counter=-1, enabled=0), task=0, m=net(D=17, A=6), packed=None) == E_NULL
    # the shape query: host-side
    sup = lib.smx_synth_eval_supported
    assert sup(0, 1, 6, 0, 32, 32, 2) == 1 and sup(0, 1, 6, 12, 32, 32, 2) == 1 and sup(1, 1, 6, 0, 32, 32, 2) == 1
    assert sup(0, 0, 17, 0, 28, 20, 6) == 1 and sup(1, 0, 17, 0, 28, 20, 6) == 1
    assert sup(0, 1, 6, 0, 30, 32, 2) == 0 and sup(0, 1, 6, 0, 32, 644, 2) == 0 and sup(0, 1, 7, 0, 32, 32, 2) == 0
    assert sup(0, 1, 66, 0, 32, 32, 22) == 0 and sup(0, 0, 17, 0, 32, 32, 33) == 0 and sup(0, 7, 6, 0, 32, 32, 2) == 0
    assert sup(1, 1, 6, 12, 32, 32, 2) == 0 and sup(0, 1, 6, 10, 32, 32, 2) == 0 and sup(0, 1, 6, 132, 32, 32, 2) == 0


def evaluate(venv, agent, E, resets=None, noise=None, apw=0):
    """venv.evaluate -> np.float64 [n, E]; resets / noise as above ((seed, counter, actor_base))"""
    kw = {}
    if resets is not None:
        kw['resets'] = (resets[0], resets[1], resets[2])
    if noise is not None:
        kw['noise'] = (noise[0], noise[1], noise[2])
    return venv.evaluate(agent, E, actors_per_workgroup=apw, **kw).cpu().numpy()
