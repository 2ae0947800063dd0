"""CPU tier: the on-device episode monitor (SyntheticVecEnv.attach_monitor) on the torch-CPU doubles of the stepping
launches against n host SyntheticEnv wrapped in EpisodeMonitor, driven by the same policy and draws as the existing
host-path helpers -- the doubles equal the host path bit for bit, so episode rewards and lengths are compared for
equality; resumability, reset(), ring overflow, the per-actor reports, the unmodified doubles, and the struct layout."""
import ctypes

import numpy as np
import pytest
import torch

import ddpg_pixel_rollout_cases as DPC
import ddpg_rollout_cases as DC
import episode_monitor_cases as EM
import lstm_rollout_cases as LC
import ppo_pixel_window_cases as PPC
import ppo_window_cases as PW
from helpers import _offsets

PIXEL = (2, 20, 24)


def _double(cls):
    from surreal_amd import kernels as KN
    prev = KN.set_default_kernels(cls(), 'cpu')
    try:
        yield KN.default_kernels()
    finally:
        KN.set_default_kernels(*prev)


@pytest.fixture
def ddpg_double():
    yield from _double(EM.DdpgMonitorCpuKernels)


@pytest.fixture
def ppo_double():
    yield from _double(EM.PpoMonitorCpuKernels)


# ---- DDPG ------------------------------------------------------------------------------------------------------------

def _ddpg(K, camera, n=3, D=5, A=2, episode_len=9, calls=(5, 7, 4), capacity=64, monitor_capacity=8, stacks=2,
          w3_scale=8.0, **cfg):
    """ddpg_rollout_into over `calls` with a monitor attached -> (venv, monitor, agent, configs, eps_all)"""
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    if camera:
        lc, ec, sc = DPC.configs(D, A, n, PIXEL, stacks, memory_size=capacity, **cfg)
    else:
        lc, ec, sc = DC.configs(D, A, n, memory_size=capacity, **cfg)
    agent = DC.make_agent(lc, ec, sc, w3_scale=w3_scale)
    eps_all = np.random.RandomState(11).randn(sum(calls), n, A).astype(np.float32)
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, device='cpu', kernels=K,
                           **(dict(pixel=PIXEL, frame_stacks=stacks) if camera else {}))
    mon = venv.attach_monitor(capacity=monitor_capacity)
    replay = UniformReplay(lc, ec, sc)
    s0 = 0
    for T in calls:
        venv.ddpg_rollout_into(agent, replay, T, eps=torch.as_tensor(eps_all[s0:s0 + T]))
        s0 += T
    return venv, mon, agent, (lc, ec, sc), eps_all


@pytest.mark.parametrize('camera', [False, True])
@pytest.mark.parametrize('noise', ['normal', 'ou_noise'])
def test_ddpg_rollout_totals_equal_the_host_monitors(ddpg_double, noise, camera):
    n, L_, cap = 3, 9, 64
    venv, mon, agent, (lc, ec, sc), eps_all = _ddpg(ddpg_double, camera, n=n, episode_len=L_, capacity=cap, n_step=3,
                                                    noise_type=noise, max_sigma=0.8)
    with EM.host_monitors() as hosts:
        if camera:
            DPC.host_ring(agent, lc, ec, sc, n, L_, eps_all, cap, PIXEL, 2)
        else:
            DC.host_ring(agent, lc, ec, sc, n, L_, eps_all, cap)
    EM.assert_equals_host(mon, hosts)
    assert mon.num_episodes == n and mon.episode_steps[0] == [L_]


def test_ddpg_per_step_path_feeds_the_monitor_too(ddpg_double):
    """a LayerNorm actor takes one forward and one step launch per step: the same episodes as the host's"""
    n, L_, cap = 3, 9, 64
    venv, mon, agent, (lc, ec, sc), eps_all = _ddpg(ddpg_double, False, n=n, episode_len=L_, capacity=cap, n_step=2,
                                                    layernorm=True)
    with EM.host_monitors() as hosts:
        DC.host_ring(agent, lc, ec, sc, n, L_, eps_all, cap)
    mon.poll()
    for a, h in enumerate(hosts):
        assert mon.episode_steps[a] == h.episode_steps
        # (batched rows against batch-1 act: test_ddpg_rollout_cpu's 1e-5 per step, L steps an episode)
        np.testing.assert_allclose(mon.episode_rewards[a], h.episode_rewards, atol=L_ * 1e-5, rtol=0)


# ---- PPO -------------------------------------------------------------------------------------------------------------

def _ppo(camera, rnn_hidden, chunks, n=3, D=5, A=2, n_step=4, stride=3, episode_len=9, monitor_capacity=8, stacks=2,
         seed=3):
    """ppo_rollout_into over `chunks` with a monitor attached, and the host path over the same draws with every
    SyntheticEnv inside an EpisodeMonitor -> (venv, monitor, host monitors)"""
    from surreal_amd.env import SyntheticVecEnv
    from surreal_amd.replay import FIFOReplay
    steps = sum(chunks)
    eps = torch.randn(steps, n, A, generator=torch.Generator().manual_seed(seed))
    make = (lambda: PPC.make_agent(D, A, n_step, stride, PIXEL, stacks, rnn_hidden=rnn_hidden, seed=seed)) if camera \
        else (lambda: PW.make_agent(D, A, n_step, stride, rnn_hidden=rnn_hidden, seed=seed))
    host_agent, cfg = make()
    with EM.host_monitors() as hosts:
        if camera:
            PPC.host_windows(host_agent, cfg, n, D, episode_len, steps, eps, PIXEL, stacks)
        else:
            PW.host_windows(host_agent, cfg, n, D, episode_len, steps, eps)
    agent, (lc, ec, sc) = make()
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, seeds=list(range(n)), device='cpu',
                           **(dict(pixel=PIXEL, frame_stacks=stacks) if camera else {}))
    mon = venv.attach_monitor(capacity=monitor_capacity)
    PW.device_windows(venv, agent, FIFOReplay(lc, ec, sc), chunks, eps)
    return venv, mon, hosts


@pytest.mark.parametrize('camera,rnn_hidden', [(False, None), (False, 12), (False, 10), (True, None), (True, 12)])
def test_ppo_window_rollout_totals_equal_the_host_monitors(ppo_double, camera, rnn_hidden):
    venv, mon, hosts = _ppo(camera, rnn_hidden, [5, 7, 4, 6])
    EM.assert_equals_host(mon, hosts)
    assert mon.num_episodes == 3 * 2 and mon.episode_steps[2] == [9, 9]


def _rollout_pair(K, rnn_hidden, n=4, D=6, A=3, T=7, rounds=2):
    """`rounds` whole-episode rollout() calls (T = episode_len) against the host path over the same draws"""
    from surreal_amd.env import SyntheticVecEnv
    eps = torch.randn(rounds * T, n, A, generator=torch.Generator().manual_seed(5))
    host_agent, cfg = PW.make_agent(D, A, T, T, rnn_hidden=rnn_hidden)
    with EM.host_monitors() as hosts:
        PW.host_windows(host_agent, cfg, n, D, T, rounds * T, eps)
    agent, _ = PW.make_agent(D, A, T, T, rnn_hidden=rnn_hidden)
    venv = SyntheticVecEnv(n, D, A, episode_len=T, seeds=list(range(n)), device='cpu')
    mon = venv.attach_monitor(capacity=4)
    tables = []
    for k in range(rounds):
        venv.start_rollout(T, info_width=2 * A)
        venv.rollout(agent, eps=eps[k * T:(k + 1) * T])
        tables.append(venv.rolls['rewards'][:, :T].clone())
    return mon, hosts, torch.cat(tables, 1)


@pytest.mark.parametrize('rnn_hidden', [None, 12])
def test_rollout_totals_equal_the_host_monitors(ppo_double, rnn_hidden):
    """rollout() on the doubles: the layered path of a plain-MLP policy (three launches a step), the one-launch double
    of an LSTM-stem one (the agent's state is not reset between the host's episodes either: PW.host_windows)"""
    T = 7
    mon, hosts, rewards = _rollout_pair(ppo_double, rnn_hidden, T=T, rounds=1 if rnn_hidden else 2)
    EM.assert_states_equal(EM.monitor_state(mon), EM.sequential_sums(rewards, 0, T, 4))
    EM.assert_equals_host(mon, hosts)


def test_raw_step_totals_equal_the_host_monitors(ppo_double):
    from surreal_amd.env import SyntheticVecEnv, EpisodeMonitor
    from surreal_amd.env.synthetic_env import SyntheticEnv
    n, D, A, L_, steps = 3, 5, 2, 4, 11
    actions = (2.0 * torch.randn(steps, n, A, generator=torch.Generator().manual_seed(9)))
    venv = SyntheticVecEnv(n, D, A, episode_len=L_, seeds=list(range(n)), device='cpu')
    mon = venv.attach_monitor(capacity=4)
    hosts = [EpisodeMonitor(SyntheticEnv(D, A, episode_len=L_, seed=a)) for a in range(n)]
    for h in hosts:
        h.reset()
    for s in range(steps):
        venv.step(actions[s].clone())
        for a, h in enumerate(hosts):
            if h.step(actions[s, a].numpy())[2]:
                h.reset()
    EM.assert_equals_host(mon, hosts)
    assert mon.num_episodes == n * 2 and int(mon.open_episodes()[1][0]) == 3


# ---- resumability, reset, overflow -----------------------------------------------------------------------------------

@pytest.mark.parametrize('camera', [False, True])
def test_split_calls_leave_the_same_monitor_as_one_call(ddpg_double, camera):
    """(5, 7, 4) steps over episodes of 9 against one call of 16"""
    kw = dict(n=3, episode_len=9, n_step=3, noise_type='ou_noise')
    _, split, *_ = _ddpg(ddpg_double, camera, calls=(5, 7, 4), **kw)
    _, whole, *_ = _ddpg(ddpg_double, camera, calls=(16,), **kw)
    EM.assert_states_equal(EM.monitor_state(split), EM.monitor_state(whole))
    assert int(whole.ep_count[0]) == 1 and int(whole.ep_steps[0]) == 7


@pytest.mark.parametrize('rnn_hidden', [None, 12])
def test_split_ppo_calls_leave_the_same_monitor_as_one_call(ppo_double, rnn_hidden):
    _, split, _ = _ppo(False, rnn_hidden, [5, 7, 4])
    _, whole, _ = _ppo(False, rnn_hidden, [16])
    EM.assert_states_equal(EM.monitor_state(split), EM.monitor_state(whole))
    assert int(whole.ep_count[0]) == 1 and int(whole.ep_steps[0]) == 7


def test_reset_drops_the_open_episode_and_keeps_the_finished(ddpg_double):
    venv, mon, *_ = _ddpg(ddpg_double, False, calls=(5, 7), episode_len=9, n_step=3)       # 12 steps: one episode + 3
    before = EM.monitor_state(mon)
    assert int(before['ep_steps'][0]) == 3 and float(before['ep_reward'][0]) != 0.0
    venv.reset()
    after = EM.monitor_state(mon)
    assert not after['ep_steps'].any() and not after['ep_reward'].any()
    for k in ('ep_count', 'done_reward', 'done_steps'):
        assert torch.equal(after[k], before[k]), k
    assert [len(x) for x in mon.episode_rewards] == [0, 0, 0]
    assert len(mon.poll()) == 3 and mon.episode_steps == [[9]] * 3


def test_ring_overflow_drops_the_oldest_and_keeps_the_order(ddpg_double):
    n, L_ = 3, 4
    kw = dict(n=n, episode_len=L_, n_step=2, capacity=128)
    _, small, *_ = _ddpg(ddpg_double, False, calls=(5 * L_ + 1,), monitor_capacity=2, **kw)
    _, large, *_ = _ddpg(ddpg_double, False, calls=(5 * L_ + 1,), monitor_capacity=8, **kw)
    new = small.poll()
    large.poll()
    assert small.dropped == 3 * n and small.dropped_by_actor == [3] * n
    assert small.num_episodes == 5 * n == large.num_episodes and large.dropped == 0
    for a in range(n):
        assert len(large.episode_rewards[a]) == 5
        assert small.episode_rewards[a] == large.episode_rewards[a][-2:]
        assert small.episode_steps[a] == [L_, L_]
    assert new == [(a, small.episode_rewards[a][i], L_) for a in range(n) for i in range(2)]
    assert small.poll() == [] and small.dropped == 3 * n


def test_polls_between_calls_report_every_episode_once(ddpg_double):
    from surreal_amd.replay import UniformReplay
    n, L_ = 2, 3
    venv, mon, agent, (lc, ec, sc), eps_all = _ddpg(ddpg_double, False, n=n, episode_len=L_, n_step=2, calls=(4,),
                                                    monitor_capacity=2)
    seen = [mon.poll()]
    replay = UniformReplay(lc, ec, sc)
    for _ in range(3):
        venv.ddpg_rollout_into(agent, replay, 4, eps=torch.zeros(4, n, 2))
        seen.append(mon.poll())
    assert [len(x) for x in seen] == [n * 1, n * 1, n * 2, n * 1]         # 16 steps: 5 episodes, 1 + 1 + 2 + 1
    assert mon.dropped == 0 and mon.num_episodes == 5 * n and mon.total_steps == 16 * n
    assert mon.mean_reward(last=2) == pytest.approx(np.mean([r for a in range(n) for r in mon.episode_rewards[a][-2:]]))


# ---- reports ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('period', [1, 2])
def test_training_monitor_reports_what_the_host_monitors_report(ddpg_double, period):
    from surreal_amd.env import DeviceTrainingMonitor, TrainingTensorplexMonitor
    n, L_ = 3, 4
    kw = dict(n=n, episode_len=L_, n_step=2, capacity=128, monitor_capacity=8, w3_scale=1.0, max_sigma=0.8)
    venv, mon, agent, (lc, ec, sc), eps_all = _ddpg(ddpg_double, False, calls=(9, 2, 10), **kw)
    sc.tensorplex.update_schedule.training_env = period
    venv2, _, *_ = _ddpg(ddpg_double, False, calls=(9,), **kw)
    reports = DeviceTrainingMonitor(venv2, sc)
    from surreal_amd.replay import UniformReplay
    replay = UniformReplay(lc, ec, sc)
    for T, s0 in ((2, 9), (10, 11)):
        venv2.ddpg_rollout_into(agent, replay, T, eps=torch.as_tensor(eps_all[s0:s0 + T]))
        reports.poll()
    with EM.host_monitors(lambda env, i: TrainingTensorplexMonitor(env, i, sc)) as hosts:
        DC.host_ring(agent, lc, ec, sc, n, L_, eps_all, 128)

    def rows(tp):
        return [(step, ':reward', s[':reward']) for step, s in tp.history]
    for a in range(n):
        got, want = rows(reports.reports[a].tensorplex), rows(hosts[a].tensorplex)
        assert got == want and len(want) == 5 // period, (a, got, want)
        assert reports.reports[a].tensorplex_name == hosts[a].tensorplex_name == 'agent/%d' % a
        assert all('step_per_s' in s for _, s in reports.reports[a].tensorplex.history)
    assert reports.step_per_s > 0
    assert reports.mean_reward(last=3) == reports.monitor.mean_reward(3)


# ---- the unmodified doubles ------------------------------------------------------------------------------------------

def test_the_existing_doubles_are_called_without_the_keyword():
    """no monitor attached: SyntheticVecEnv calls the doubles that know no `monitor` as before; attached: it passes it"""
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.replay import UniformReplay, FIFOReplay
    from cpu_kernels import TorchCpuKernels
    for K in _double(DC.DdpgRolloutCpuKernels):
        lc, ec, sc = DC.configs(5, 2, 3, memory_size=64, n_step=2)
        agent = DC.make_agent(lc, ec, sc)
        venv = SyntheticVecEnv(3, 5, 2, episode_len=4, device='cpu', kernels=K)
        assert venv.monitor is None
        assert venv.ddpg_rollout_into(agent, UniformReplay(lc, ec, sc), 6, eps=torch.zeros(6, 3, 2)) > 0
        venv.attach_monitor()
        with pytest.raises(TypeError, match='monitor'):
            venv.ddpg_rollout_into(agent, UniformReplay(lc, ec, sc), 6, eps=torch.zeros(6, 3, 2))
        assert venv.detach_monitor() is not None and venv.monitor is None
        assert venv.ddpg_rollout_into(agent, UniformReplay(lc, ec, sc), 2, eps=torch.zeros(2, 3, 2)) > 0
    for K in _double(PW.PpoWindowCpuKernels):
        agent, (lc, ec, sc) = PW.make_agent(5, 2, 3, 2)
        venv = SyntheticVecEnv(3, 5, 2, episode_len=4, seeds=[0, 1, 2], device='cpu')
        got, rows = PW.device_windows(venv, agent, FIFOReplay(lc, ec, sc), [6], torch.zeros(6, 3, 2))
        assert rows > 0
    for K in _double(LC.LstmRolloutCpuKernels):
        agent, _ = LC.make_agent(5, 2, T=4, n=3)
        LC.run(agent, 3, 5, 2, 4, 4, torch.zeros(4, 3, 2))
    for K in _double(TorchCpuKernels):
        venv = SyntheticVecEnv(3, 5, 2, episode_len=4, device='cpu')
        venv.step(torch.zeros(3, 2))
        assert venv.t == 1


# ---- the C ABI -------------------------------------------------------------------------------------------------------

def test_monitor_struct_matches_the_ctypes_mirror(tmp_path):
    from surreal_amd import _lib as L
    got = _offsets(tmp_path, 'struct smx_episode_monitor', L.EpisodeMonitor)
    assert got['sizeof'] == ctypes.sizeof(L.EpisodeMonitor) == 48
    for fname, _ in L.EpisodeMonitor._fields_:
        assert got[fname] == getattr(L.EpisodeMonitor, fname).offset, fname
    # embedded last in every argument block that steps the environment
    for cname, cls in (('smx_synth_rollout_t', L.SynthRollout), ('smx_ddpg_rollout_t', L.DdpgRollout),
                       ('smx_synth_act_step_t', L.SynthActStep),
                       ('struct smx_synth_ppo_pixel_window_step', L.SynthPpoPixelWindowStep)):
        assert cls._fields_[-1][0] == 'mon'
        sub = tmp_path / cname.replace(' ', '_')
        sub.mkdir()
        assert _offsets(sub, cname, cls)['mon'] == cls.mon.offset, cname


SMX_E_NULL, SMX_E_SHAPE = -1, -2


def test_half_a_monitor_is_refused_before_any_launch():
    """all five pointers or none, and a ring of at least one slot (host-side checks: no GPU needed)"""
    from surreal_amd import _lib as L
    lib = L.load()
    fake = ctypes.c_void_p(4096)

    def mon(capacity=4, **drop):
        m = L.EpisodeMonitor()
        for f in ('ep_reward', 'ep_steps', 'ep_count', 'done_reward', 'done_steps'):
            setattr(m, f, None if f in drop else fake)
        m.capacity = capacity
        return m

    def step(m):
        return lib.smx_synth_env_step_f32(fake, fake, fake, 2, 4, 2, 0, 5, 0, 1, None, None, None, None,
                                          ctypes.byref(m), None)
    assert step(mon(done_steps=1)) == SMX_E_NULL and step(mon(ep_count=1)) == SMX_E_NULL
    assert step(mon(capacity=0)) == SMX_E_SHAPE
    p = L.DdpgRollout()
    for f in ('state', 'init_state', 'gpow', 'carry_obs', 'carry_act', 'carry_rew', 'obs', 'obs_next', 'actions',
              'rewards', 'dones'):
        setattr(p, f, fake)
    p.n, p.D, p.A, p.steps, p.n_step, p.episode_len, p.capacity = 2, 4, 2, 1, 1, 5, 8
    p.mon = mon(ep_steps=1)
    assert lib.smx_synth_ddpg_step_f32(ctypes.byref(p), fake, 2, None) == SMX_E_NULL
    p.mon = mon(capacity=-1)
    assert lib.smx_synth_ddpg_step_f32(ctypes.byref(p), fake, 2, None) == SMX_E_SHAPE
