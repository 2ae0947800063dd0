"""GPU tier (-m gpu): the record launches (smx_record_ppo_window_step_f32 / smx_record_ddpg_nstep_step_f32) behind
DeviceWindowRecorder / DeviceNStepRecorder against n host wrappers stepped in actor order -- bit for bit: these are
copies, and for DDPG the same fp64 sums in the same order --, against the layout ppo_rollout_into is held to, the host
EpisodeMonitor, and end to end from HostVecEnv through the replays to the learners."""
import numpy as np
import pytest
import torch

import ppo_window_cases as PW
import recorder_cases as RC

pytestmark = pytest.mark.gpu

LENGTHS = [2, 4, 9, 5, 14]             # for N = 4: shorter than N, equal to N, closing on the terminal step, long
LONG = [12, 25, 45, 30, 65]            # the same four kinds of episode for N = 25, advance 20
DDPG_LENGTHS = [2, 3, 9, 5, 14]


@pytest.mark.parametrize('n,D,A,n_step,stride,Hl,lengths,steps,copy_workgroups', [
    (5, 7, 3, 4, 3, 0, LENGTHS, 60, 0),
    (5, 8, 3, 4, 3, 0, LENGTHS, 60, 0),             # 16-byte observation rows
    (5, 7, 3, 4, 6, 0, LENGTHS, 60, 0),             # advance = 4
    (5, 7, 3, 4, 3, 6, LENGTHS, 60, 0),             # two cell slots
    (9, 376, 17, 25, 20, 0, LENGTHS, 120, 0),       # no episode reaches n_step: nothing may be written
    (9, 376, 17, 25, 20, 0, LONG, 120, 0),          # several workgroups per closing actor
    (5, 8, 4, 4, 3, 8, LENGTHS, 60, 3),             # every field in 16-byte accesses, three workgroups per actor
    (5, 7, 3, 1, 1, 6, LENGTHS, 30, 0),             # n_step 1: a window is the step's inputs alone
])
def test_ppo_windows_equal_n_host_wrappers(n, D, A, n_step, stride, Hl, lengths, steps, copy_workgroups):
    st = RC.host_ppo(n, D, A, lengths, steps, n_step, stride, rnn_hidden=Hl)
    replay = RC.fifo(D, A, n_step, stride, 4096, rnn_hidden=Hl)
    rec, rows = RC.device_ppo(st, replay, n_step, stride, copy_workgroups=copy_workgroups)
    torch.cuda.synchronize()
    assert rows == len(st.exps) == replay.cumulative_collected_count
    assert (rows == 0) == (max(lengths) < n_step)
    RC.assert_ring_equals(replay, st.fields, 4096 + 3)
    last = np.where(st.dones[-1][:, None], st.obs_reset[-1], st.obs_next[-1])
    assert torch.equal(rec.observation.cpu(), torch.as_tensor(last))


def test_ppo_ring_wrap_pops_what_the_host_fifo_pops():
    RC.check_ring_wrap()


def test_equal_clocks_give_the_layout_of_the_synthetic_rollout():
    """every actor on the same clock: the step stream of a SyntheticVecEnv rollout table, recorded step by step, must
    be byte for byte what cut_windows cuts from that table -- the layout ppo_rollout_into is held to"""
    from surreal_amd.env import SyntheticVecEnv, DeviceWindowRecorder
    n, D, A, n_step, stride, L_ = 6, 11, 3, 7, 3, 19
    agent, cfg = PW.make_agent(D, A, n_step, stride)
    venv = SyntheticVecEnv(n, D, A, episode_len=L_, seeds=list(range(n)))
    venv.start_rollout(L_, info_width=2 * A)
    venv.rollout(agent, eps=torch.randn(L_, n, A, generator=torch.Generator().manual_seed(2)).cuda())
    table = {k: v.clone() for k, v in venv.rolls.items()}
    want, terminal = PW.cut_windows(table, 0, L_, n_step, stride)
    assert terminal and terminal[-1]                                  # (19 - 7) % 3 == 0: a window closes on the last step
    replay = RC.fifo(D, A, n_step, stride, 4096)
    rec = DeviceWindowRecorder(n, D, A, n_step, stride)
    rec.begin(table['obs'][:, 0])
    rows = 0
    for s in range(L_):
        assert torch.equal(rec.observation, table['obs'][:, s])
        done = np.full(n, s == L_ - 1)
        assert bool(table['dones'][0, s]) == (s == L_ - 1)
        rows += rec.record(replay, table['actions'][:, s].contiguous(), table['pds'][:, s].contiguous(),
                           table['rewards'][:, s].contiguous(), done, table['obs'][:, s + 1].contiguous(),
                           venv.init_state)
    torch.cuda.synchronize()
    assert rows == want['obs'].shape[0] == n * PW.closing_count(0, L_, L_, n_step, stride)
    for k, w in want.items():
        got = replay._tables[k].data[:rows]
        assert torch.equal(got, w.reshape(rows, -1)), k
    assert torch.equal(rec.observation, venv.init_state) and rec.t.tolist() == [0] * n


@pytest.mark.parametrize('n_step,D,A', [(1, 7, 3), (3, 7, 3), (5, 7, 3), (3, 8, 4)])
def test_ddpg_transitions_equal_n_host_wrappers(n_step, D, A):
    n, steps, gamma = 5, 60, 0.99
    st = RC.host_ddpg(n, D, A, DDPG_LENGTHS, steps, n_step, gamma)
    replay = RC.uniform(D, A, n, n_step, gamma, 17)
    rec, rows = RC.device_ddpg(st, replay, n_step, gamma)
    torch.cuda.synchronize()
    assert rows == len(st.exps) > 17                                  # the ring of 17 wrapped
    # an episode of T steps emits max(T - n_step + 1, 0) transitions: the short ones nothing
    finished = sum(max(T - n_step + 1, 0) for m in st.monitors for T in m.episode_steps)
    assert finished <= rows <= finished + n * 14
    RC.assert_ring_equals(replay, st.fields, 17)                      # rewards: np.float32 of the wrapper's Python float


def test_done_step_restarts_the_clock_and_resumes_from_a_state_dict():
    from surreal_amd.env import DeviceWindowRecorder
    n, D, A, n_step, stride, steps, Hl = 5, 7, 3, 4, 3, 60, 6
    st = RC.host_ppo(n, D, A, LENGTHS, steps, n_step, stride, rnn_hidden=Hl)
    replay = RC.fifo(D, A, n_step, stride, 4096, rnn_hidden=Hl)
    rec = DeviceWindowRecorder(n, D, A, n_step, stride, rnn_hidden=Hl)
    rec.begin(st.first)
    seen = []
    for s in range(steps):
        rec.record(replay, RC._dev(st.actions[s]), RC._dev(st.pds[s]), st.rewards[s], st.dones[s], st.obs_next[s],
                   st.obs_reset[s], cells_before=(RC._dev(st.h[s]), RC._dev(st.c[s])))
        seen.append(rec.observation.clone())
        assert not rec.t[st.dones[s]].any() and (rec.t[~st.dones[s]] > 0).all()
    torch.cuda.synchronize()
    for s in range(steps):                         # the reset observation where done, the next one elsewhere
        want = np.where(st.dones[s][:, None], st.obs_reset[s], st.obs_next[s])
        assert torch.equal(seen[s].cpu(), torch.as_tensor(want)), s
    assert st.dones.sum() > 10
    RC.assert_ring_equals(replay, st.fields, 4096 + 3)            # ... and the closing windows the TERMINAL ones
    resumed = RC.fifo(D, A, n_step, stride, 4096, rnn_hidden=Hl)
    rec2, rows = RC.device_ppo(st, resumed, n_step, stride, resume_at=(7, 8, 31))
    assert rows == len(st.exps)
    RC.assert_ring_equals(resumed, st.fields, 4096 + 3)
    a, b = rec.state_dict(), rec2.state_dict()
    assert a['t'].tolist() == b['t'].tolist() and torch.equal(a['cur_obs'], b['cur_obs'])
    for k in a['carry']:
        assert torch.equal(a['carry'][k], b['carry'][k]), k
    sd = RC.host_ddpg(n, D, A, DDPG_LENGTHS, steps, 3, 0.99)
    replay = RC.uniform(D, A, n, 3, 0.99, 4096)
    RC.device_ddpg(sd, replay, 3, 0.99, resume_at=(5, 40))
    RC.assert_ring_equals(replay, sd.fields, 4096)


def test_device_tensors_are_taken_where_host_arrays_are():
    n, D, A, n_step, stride, steps = 5, 8, 3, 4, 3, 30
    st = RC.host_ppo(n, D, A, LENGTHS, steps, n_step, stride)
    replay = RC.fifo(D, A, n_step, stride, 4096)
    RC.device_ppo(st, replay, n_step, stride, as_tensors=True)
    RC.assert_ring_equals(replay, st.fields, 4096 + 3)


def test_monitor_equals_the_host_monitors():
    from surreal_amd.env import DeviceEpisodeMonitor
    n, D, A, steps = 5, 7, 3, 60
    st = RC.host_ppo(n, D, A, LENGTHS, steps, 4, 3)
    mon = DeviceEpisodeMonitor(n, 32, 'cuda')
    RC.device_ppo(st, RC.fifo(D, A, 4, 3, 4096), 4, 3, monitor=mon)
    RC.assert_monitor_equals_host(mon, st)
    assert mon.total_steps == n * steps
    sd = RC.host_ddpg(n, D, A, DDPG_LENGTHS, steps, 3, 0.99)
    mon = DeviceEpisodeMonitor(n, 32, 'cuda')
    RC.device_ddpg(sd, RC.uniform(D, A, n, 3, 0.99, 4096), 3, 0.99, monitor=mon)
    RC.assert_monitor_equals_host(mon, sd)


def _host_count(wrap, n, D, lengths, T, seed, action):
    """the experiences n host wrappers emit over T steps of the same scripted environments (the count depends on the
    episode lengths alone)"""
    sent = []
    ws = [wrap(RC.ScriptedEnv(seed + a, lengths, D, rotation=a), sent.append) for a in range(n)]
    for w in ws:
        w.reset()
    for _ in range(T):
        for w in ws:
            if w.step(action)[2]:
                w.reset()
    return len(sent)


def test_host_vec_env_to_fifo_to_ppo_learn():
    from surreal_amd import synthetic
    from surreal_amd.env import (HostVecEnv, DeviceWindowRecorder, DeviceEpisodeMonitor,
                                 ExpSenderWrapperMultiStepMovingWindowWithInfo)
    from surreal_amd.learner import PPOLearner
    from surreal_amd.replay import FIFOReplay
    n, D, A, T, lengths = 6, 17, 6, 300, [30, 45, 26, 70]
    agent, (lc, ec, sc) = PW.make_agent(D, A, 25, 20, hidden=(300, 200), rnn_hidden=100, memory_size=512, batch_size=64)
    learner = PPOLearner(lc, ec, sc)
    learner.model.load_params(synthetic.make_ppo_params(D, A, hidden=(300, 200), seed=9, rnn_hidden=100))
    replay = FIFOReplay(lc, ec, sc)
    venv = HostVecEnv([RC.ScriptedEnv(90 + a, lengths, D, rotation=a) for a in range(n)])
    rec = DeviceWindowRecorder(n, D, A, 25, 20, rnn_hidden=100)
    mon = DeviceEpisodeMonitor(n, 32, 'cuda')
    written = venv.run_ppo(agent, rec, replay, T // 2, monitor=mon) + venv.run_ppo(agent, rec, replay, T // 2, monitor=mon)
    torch.cuda.synchronize()
    once = [np.zeros((1, 100), np.float32)] * 2
    want = _host_count(lambda env, sink: ExpSenderWrapperMultiStepMovingWindowWithInfo(env, lc, sc, sink=sink), n, D,
                       lengths, T, 90, (np.zeros(A, np.float32), [once, [np.zeros(2 * A, np.float32)]]))
    assert written == want == replay.cumulative_collected_count and want >= 64
    mon.poll()
    assert [len(x) for x in mon.episode_steps] == [e.episode - 1 for e in venv.envs]
    assert all(s in lengths for per_actor in mon.episode_steps for s in per_actor)
    stats = learner.learn(venv.to_batch(replay.sample_batch(64, copy=False)))
    for k, v in stats.items():
        assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k
    assert len(replay) == written - 64


def test_host_vec_env_to_uniform_replay_with_ddpg():
    import ddpg_rollout_cases as DC
    from surreal_amd.env import HostVecEnv, DeviceNStepRecorder, ExpSenderWrapperSSARNStepBootstrap
    from surreal_amd.replay import UniformReplay
    n, D, A, T, N = 6, 17, 6, 60, 3
    lc, ec, sc = DC.configs(D, A, n, hidden=(300, 200), n_step=N, memory_size=4096, folder='surreal_amd_recorder')
    agent = DC.make_agent(lc, ec, sc, w3_scale=1.0)
    replay = UniformReplay(lc, ec, sc)
    venv = HostVecEnv([RC.ScriptedEnv(40 + a, DDPG_LENGTHS, D, rotation=a) for a in range(n)])
    rec = DeviceNStepRecorder(n, D, A, N, lc.algo.gamma)
    written = venv.run_ddpg(agent, rec, replay, T, sigmas=agent.batch_sigmas(n).float())
    torch.cuda.synchronize()
    want = _host_count(lambda env, sink: ExpSenderWrapperSSARNStepBootstrap(env, lc, sc, sink=sink), n, D, DDPG_LENGTHS, T,
                       40, np.zeros(A, np.float32))
    assert written == want == replay.cumulative_collected_count == len(replay) > 100
    batch = replay.sample_batch(32)
    assert tuple(batch['obs'].shape) == (32, D) and tuple(batch['actions'].shape) == (32, A)
    for k, v in batch.items():
        assert torch.isfinite(v).all(), k
    assert (batch['actions'].abs() <= 1).all() and set(batch['dones'].unique().tolist()) <= {0.0, 1.0}
    assert batch['obs'].abs().sum(1).min() > 0                        # every sampled row holds a transition
