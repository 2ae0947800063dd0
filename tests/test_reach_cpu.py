"""CPU tier: the `reach` task (surreal_amd/env/tasks.py).  The host env against a float64 restatement; the PD controller
against the zero action; task='drift' leaves the bytes of no keyword; the torch-CPU doubles of the task entry points
against n host chains -- SyntheticEnv(task='reach') behind the project's windowing and n-step wrappers -- bit for bit and
against the float64 restatement within the project's 1e-5; the refusal table; the header's defines."""
import os
import re
import types

import numpy as np
import pytest
import torch

import ddpg_rollout_cases as DC
import helpers as H
import ppo_window_cases as PW
import reach_cases as RC
import rollout_envelope_cases as EC
from reach_cpu_kernels import ReachCpuKernels
from surreal_amd import _lib as L
from surreal_amd.env import tasks as TK
from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def double():
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(ReachCpuKernels(), 'cpu')
    yield KN.default_kernels()
    KN.set_default_kernels(*prev)


# ---- the host definition -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('A', [1, 2, 21])
def test_host_env_against_the_float64_restatement(A):
    """two episodes of 10 steps under actions that reach past the clip.  Bound: the project's 1e-5 (absolute plus
    relative).  A step rounds each of its at most four fp32 operations to 2^-24 relative on values below 10, so ten
    steps from an exact reset state stay under 10 x 4 x 6e-8 x 10 = 2.4e-5 in the worst case and a hundredth of that
    typically; the reward's fp64 sums add nothing to it"""
    L_, D = 10, 3 * A
    env = SyntheticEnv(D, A, episode_len=L_, seed=5, task='reach')
    env._reset()
    ref = RC.ReachEnv(env.init_state[None], A, L_)
    acts = np.random.RandomState(A).randn(2 * L_, A).astype(np.float32) * 1.5
    for s in range(2 * L_):
        before, sn, rew, done = ref.step(RC.R.f64(acts[s][None]))
        obs, r, d, _ = env._step(acts[s])
        assert d == done
        got = obs['low_dim']['flat_inputs']
        assert got.dtype == np.float32
        np.testing.assert_allclose(got, sn[0].numpy(), atol=1e-5, rtol=1e-5)
        np.testing.assert_allclose(r, float(rew[0]), atol=1e-5, rtol=1e-5)
        assert np.array_equal(got[2 * A:], env.init_state[2 * A:])           # the goals never move
        if d:
            obs, _ = env._reset()
            assert np.array_equal(obs['low_dim']['flat_inputs'], env.init_state)
    assert len(ref.finished) == 2


def test_reach_step_batches_rows_with_the_same_bits():
    rs = np.random.RandomState(0)
    s, a = rs.randn(7, 63).astype(np.float32), rs.randn(7, 21).astype(np.float32)
    sn, r = TK.reach_step(s, a)
    for i in range(7):
        sni, ri = TK.reach_step(s[i], a[i])
        assert np.array_equal(sn[i], sni) and r[i] == ri and r.dtype == np.float32


def test_pd_controller_beats_the_zero_action():
    J, L_, seeds = 2, 50, range(64)
    zero = RC.host_returns(J, L_, seeds, lambda s: np.zeros(J, np.float32))
    pd = RC.host_returns(J, L_, seeds, TK.reach_pd_action)
    assert pd.mean() > zero.mean() and (pd > zero).all()


def test_env_refuses_what_the_task_cannot_be():
    for make in (lambda **kw: SyntheticEnv(**kw), lambda **kw: SyntheticVecEnv(4, device='cpu', kernels=ReachCpuKernels(), **kw)):
        with pytest.raises(ValueError, match='3 \\* action_dim'):
            make(obs_dim=7, action_dim=2, task='reach')
        with pytest.raises(ValueError, match='no camera'):
            make(obs_dim=6, action_dim=2, task='reach', pixel=(1, 8, 8))
        with pytest.raises(ValueError, match='task must be one of'):
            make(obs_dim=6, action_dim=2, task='pendulum')
        assert make(obs_dim=66, action_dim=22, task='reach').task == 'reach'         # (the host has no width limit)
        assert make(obs_dim=7, action_dim=2).task == 'drift'


# ---- 'drift' is what it was -----------------------------------------------------------------------------------------------

def test_drift_keyword_leaves_the_same_bytes_on_the_host():
    a, b = SyntheticEnv(7, 3, episode_len=4, seed=2), SyntheticEnv(7, 3, episode_len=4, seed=2, task='drift')
    acts = np.random.RandomState(1).randn(9, 3).astype(np.float32)
    a._reset(), b._reset()
    for s in range(9):
        (oa, ra, da, _), (ob, rb, db, _) = a._step(acts[s]), b._step(acts[s])
        assert np.array_equal(oa['low_dim']['flat_inputs'], ob['low_dim']['flat_inputs']) and ra == rb and da == db
        if da:
            a._reset(), b._reset()


@pytest.mark.parametrize('c', [RC.CASES[1], RC.CASES[3], RC.CASES[6]], ids=lambda c: c.id)
def test_drift_keyword_leaves_the_same_bytes_on_the_doubles(double, c):
    """task='drift' on the double that takes tasks against no keyword on the doubles that know none: were the keyword
    passed for 'drift', those would raise"""
    plain = DC.DdpgRolloutCpuKernels() if c.family == 'ddpg' else PW.PpoWindowCpuKernels()
    got, rows = RC.run(RC.setup(c, 'cpu', ReachCpuKernels(), task='drift'))
    want, wrows = RC.run(RC.setup(c, 'cpu', plain, task=None))
    assert rows == wrows > 0
    EC.same_bits(got, want)
    venv = SyntheticVecEnv(3, 6, 2, episode_len=2, device='cpu', kernels=PW.PpoWindowCpuKernels(), task='drift')
    ref = SyntheticVecEnv(3, 6, 2, episode_len=2, device='cpu', kernels=PW.PpoWindowCpuKernels())
    acts = torch.randn(3, 2, generator=torch.Generator().manual_seed(0))
    for _ in range(3):
        assert torch.equal(venv.step(acts), ref.step(acts))


# ---- the doubles against n host chains -------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_step,stride,rnn_hidden,episode_len,chunks', [
    (3, 2, None, 5, [4, 5, 3]),                  # two episode ends inside; a window closes at the terminal step
    (3, 2, 8, 5, [4, 5, 3]),                     # one LSTM layer
    (25, 20, None, 53, [17, 40, 33, 29]),        # the reference default windows
])
def test_windowed_double_matches_the_host_chains_bit_for_bit(double, n_step, stride, rnn_hidden, episode_len, chunks):
    from surreal_amd.replay import FIFOReplay
    n, D, A = 3, 6, 2
    steps = sum(chunks)
    eps = torch.randn(steps, n, A, generator=torch.Generator().manual_seed(3))
    host_agent, cfg = PW.make_agent(D, A, n_step, stride, rnn_hidden=rnn_hidden)
    with RC.reach_host_envs():
        want = PW.host_windows(host_agent, cfg, n, D, episode_len, steps, eps)
    agent, (lc, ec, sc) = PW.make_agent(D, A, n_step, stride, rnn_hidden=rnn_hidden)
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, seeds=list(range(n)), device='cpu', task='reach')
    got, rows = PW.device_windows(venv, agent, FIFOReplay(lc, ec, sc), chunks, eps)
    assert rows == len(want['obs']) > 0 and double.window_launches == len(chunks)
    for k, w in want.items():
        g = got[k].reshape(w.shape)
        assert np.array_equal(g.view(np.uint32), w.astype(np.float32).view(np.uint32)), k
    # and they are not the drift's windows
    drift = SyntheticVecEnv(n, D, A, episode_len=episode_len, seeds=list(range(n)), device='cpu')
    agent2, (lc, ec, sc) = PW.make_agent(D, A, n_step, stride, rnn_hidden=rnn_hidden)
    other, _ = PW.device_windows(drift, agent2, FIFOReplay(lc, ec, sc), chunks, eps)
    assert not np.array_equal(other['rewards'], got['rewards'])


@pytest.mark.parametrize('noise', ['ou_noise', 'normal', 'deterministic'])
def test_ddpg_double_matches_the_host_chains_bit_for_bit(double, noise):
    from surreal_amd.replay import UniformReplay
    n, D, A, episode_len, calls, capacity = 3, 6, 2, 9, (5, 7, 4), 23
    mode = 'eval_deterministic_local' if noise == 'deterministic' else 'training'
    lc, ec, sc = DC.configs(D, A, n, memory_size=capacity, n_step=3, max_sigma=0.8,
                            noise_type='normal' if noise == 'deterministic' else noise)
    agent = DC.make_agent(lc, ec, sc, mode=mode)
    eps_all = np.random.RandomState(11).randn(sum(calls), n, A).astype(np.float32)
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, device='cpu', task='reach')
    replay = UniformReplay(lc, ec, sc)
    written, s0 = 0, 0
    for T in calls:
        written += venv.ddpg_rollout_into(agent, replay, T, eps=torch.as_tensor(eps_all[s0:s0 + T]))
        s0 += T
    with RC.reach_host_envs():
        want, total = DC.host_ring(agent, lc, ec, sc, n, episode_len, eps_all, capacity)
    assert written == total > capacity                           # the ring wrapped
    got = H.device_ring(replay, DC.FIELDS)
    for k in DC.FIELDS:
        g, w = got[k].reshape(want[k].shape), want[k]
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (k, np.argwhere(g != w)[:5])


def test_step_double_matches_the_host_env_bit_for_bit(double):
    n, D, A, L_ = 5, 6, 2, 3
    venv = SyntheticVecEnv(n, D, A, episode_len=L_, device='cpu', task='reach')
    mon = venv.attach_monitor(capacity=4)
    hosts = [SyntheticEnv(D, A, episode_len=L_, seed=a, task='reach') for a in range(n)]
    returns = [[0.0] for _ in range(n)]
    acts = torch.randn(7, n, A, generator=torch.Generator().manual_seed(4)) * 1.5
    for s in range(7):
        state = venv.step(acts[s]).clone()
        for a, h in enumerate(hosts):
            obs, r, done, _ = h._step(acts[s, a].numpy())
            returns[a][-1] += r
            if done:
                obs, _ = h._reset()
                returns[a].append(0.0)
            assert np.array_equal(state[a].numpy(), obs['low_dim']['flat_inputs'])
    # the monitor's finished episodes: the host's sums of the same fp32 rewards, to the bit
    assert mon.ep_count.tolist() == [2] * n and mon.done_steps[:, :2].eq(L_).all()
    assert mon.done_reward[:, :2].tolist() == [r[:2] for r in returns]
    assert mon.ep_reward.tolist() == [r[2] for r in returns]


# ---- the doubles and the restatement: where the GPU tier's seeds come from ---------------------------------------------------

@pytest.mark.parametrize('c', RC.CASES, ids=lambda c: c.id)
def test_restatement_meets_its_input_conditions_and_the_double_meets_it(double, c):
    c = RC.tuned(c)
    x = RC.setup(c, 'cpu', ReachCpuKernels(), wrap=False)
    want, wrows, written, pol = RC.restatement(x)
    print(c.id, RC.input_conditions(pol))
    got, rows = RC.run(x)
    assert rows == wrows == x.rows
    errs = EC.worst_errors(got, want, written)
    print(c.id, {k: round(v, 3) for k, v in errs.items()})
    assert max(errs.values()) <= 1.0, errs


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def fake_agent(**model):
    return types.SimpleNamespace(model=types.SimpleNamespace(**model),
                                 rnn_config=types.SimpleNamespace(if_rnn_policy=False, rnn_layer=1))


def test_task_env_refuses_every_other_stepping_call_and_route(double):
    venv = SyntheticVecEnv(4, 6, 2, episode_len=5, device='cpu', task='reach')
    agent, (lc, ec, sc) = PW.make_agent(6, 2, 3, 2, hidden=(8, 4))
    refused = dict(match="task 'reach' is stepped by step")
    for call in (lambda: venv.start_rollout(4), lambda: venv.rollout(agent), lambda: venv.rollout_into(agent, {}),
                 lambda: venv.rollout_reference(agent, None), lambda: venv.emit_windows(3, 2)):
        with pytest.raises(NotImplementedError, **refused):
            call()
    # PPO: a camera agent, two LSTM layers, per-actor clocks; a policy shape the kernel does not take
    with pytest.raises(NotImplementedError, **refused):
        venv.ppo_rollout_into(fake_agent(if_pixel=True), None, 4)
    two, _ = PW.make_agent(6, 2, 3, 2, hidden=(8, 4), rnn_hidden=8)
    two.rnn_config.rnn_layer = 2
    with pytest.raises(NotImplementedError, **refused):
        venv.ppo_rollout_into(two, None, 4)
    clocked = SyntheticVecEnv(4, 6, 2, episode_len=[5, 5, 4, 3], device='cpu', task='reach')
    with pytest.raises(NotImplementedError, **refused):
        clocked.ppo_rollout_into(agent, None, 4)
    odd, _ = PW.make_agent(6, 2, 3, 2, hidden=(6, 4))
    assert not venv.can_ppo_rollout_into(odd)
    with pytest.raises(ValueError, match='policy shapes the persistent kernel refuses'):
        venv.ppo_rollout_into(odd, None, 4)
    # DDPG: a camera agent, a LayerNorm actor, a parameter noise, per-actor clocks, the 'two_launch' and 'steps' routes
    dl, de, ds = DC.configs(6, 2, 4, hidden=(8, 4))
    plain = DC.make_agent(dl, de, ds)
    with pytest.raises(NotImplementedError, **refused):
        venv.ddpg_rollout_into(fake_agent(is_pixel_input=True), None, 4)
    with pytest.raises(NotImplementedError, **refused):
        venv.ddpg_rollout_into(DC.make_agent(*DC.configs(6, 2, 4, hidden=(8, 4), layernorm=True)), None, 4)
    venv.param_noise = object()
    with pytest.raises(NotImplementedError, **refused):
        venv.ddpg_rollout_into(plain, None, 4)
    venv.param_noise = None
    with pytest.raises(NotImplementedError, **refused):
        clocked.ddpg_rollout_into(plain, None, 4)
    with pytest.raises(NotImplementedError, **refused):
        venv.ddpg_rollout_into(plain, None, 4, reference=True)
    with pytest.raises(NotImplementedError, **refused):
        venv.ddpg_rollout_into(DC.make_agent(*DC.configs(6, 2, 4, hidden=(6, 4))), None, 4)
    with pytest.raises(NotImplementedError, match='per-actor episode clocks'):
        clocked.step(torch.zeros(4, 2))
    # nothing above stepped anything
    assert torch.equal(venv.state, venv.init_state) and venv.t == 0


def test_task_env_refuses_more_than_21_actions(double):
    venv = SyntheticVecEnv(4, 66, 22, episode_len=5, device='cpu', task='reach')
    with pytest.raises(ValueError, match='action_dim <= 21'):
        venv.step(torch.zeros(4, 22))
    agent, (lc, ec, sc) = PW.make_agent(66, 22, 3, 2, hidden=(8, 4))
    with pytest.raises(ValueError, match='action_dim <= 21'):
        venv.ppo_rollout_into(agent, None, 4)
    with pytest.raises(ValueError, match='action_dim <= 21'):
        venv.ddpg_rollout_into(DC.make_agent(*DC.configs(66, 22, 4, hidden=(8, 4))), None, 4)


def test_task_supported_answers_from_the_built_library():
    lib = L.load()
    table = {(1, 3, 1): 1, (1, 63, 21): 1, (1, 66, 22): 0, (1, 7, 2): 0, (0, 376, 17): 1, (7, 3, 1): 0}
    for args, want in table.items():
        assert lib.smx_synth_task_supported(*args) == want, args
    K = ReachCpuKernels()
    assert K.synth_task_supported('reach', 63, 21) and not K.synth_task_supported('reach', 66, 22)


def test_task_entry_points_refuse_before_any_launch():
    """an unknown task and shapes the task does not take: SMX_E_UNSUPPORTED from argument blocks whose pointers are never
    read (no GPU here: a launch would fail otherwise)"""
    lib = L.load()
    fake = L.c_void_p(4096)
    step = lambda D, A, task: lib.smx_synth_task_env_step_f32(fake, fake, fake, 4, D, A, 0, 5, 0, 1, None, None, None, None,  # noqa: E731
                                                              None, task, None)
    assert step(6, 2, 7) == L.SMX_E_UNSUPPORTED and step(7, 2, 1) == L.SMX_E_UNSUPPORTED
    assert step(66, 22, 1) == L.SMX_E_UNSUPPORTED
    p, d = L.SynthPpoWindowRollout(), L.DdpgRollout()
    assert lib.smx_synth_ppo_window_rollout_task_f32(p, 7, None) == L.SMX_E_UNSUPPORTED
    assert lib.smx_synth_ddpg_rollout_task_f32(d, 7, None) == L.SMX_E_UNSUPPORTED
    assert lib.smx_synth_ppo_window_rollout_task_f32(None, 1, None) != 0
    assert lib.smx_synth_ddpg_rollout_task_f32(None, 1, None) != 0


def test_header_defines_match_the_bindings():
    hdr = open(os.path.join(ROOT, 'include', 'surreal_amd.h')).read()
    got = tuple(int(re.search(r'#define %s (\d+)' % k, hdr).group(1)) for k in ('SMX_TASK_DRIFT', 'SMX_TASK_REACH'))
    assert got == (L.SMX_TASK_DRIFT, L.SMX_TASK_REACH) == (TK.TASK_IDS['drift'], TK.TASK_IDS['reach'])
    assert L.load().smx_abi_version() == 2
