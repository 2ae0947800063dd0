"""CPU tier: the device recorders' host logic (per-actor clocks, ranks, staging, state) on the torch-CPU double of the two
record entry points, against n host wrappers; the rank arithmetic against brute force; the refusals; HostVecEnv's
stepping order; and the argument structs and checks of the C entry points, which refuse a bad call before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import recorder_cases as RC
from helpers import _offsets

LENGTHS = [2, 4, 9, 5, 14]             # shorter than N, equal to N, closing on the terminal step, long
DDPG_LENGTHS = [2, 3, 9, 5, 14]
SMX_E_NULL, SMX_E_SHAPE = -1, -2


@pytest.fixture
def double():
    from surreal_amd import kernels as KN
    K = RC.RecorderCpuKernels()
    prev = KN.set_default_kernels(K, 'cpu')
    yield K
    KN.set_default_kernels(*prev)


# ---- windows and transitions against the host wrappers -----------------------------------------------------------------
@pytest.mark.parametrize('D,n_step,stride,Hl', [(7, 4, 3, 0), (8, 4, 3, 0), (7, 4, 6, 0), (7, 4, 3, 6)])
def test_ppo_windows_equal_n_host_wrappers(double, D, n_step, stride, Hl):
    n, A, steps = 5, 3, 60
    st = RC.host_ppo(n, D, A, LENGTHS, steps, n_step, stride, rnn_hidden=Hl)
    assert len(st.exps) > 20 and len({m.num_episodes for m in st.monitors}) > 1          # the clocks diverged
    replay = RC.fifo(D, A, n_step, stride, 4096, rnn_hidden=Hl)
    rec, rows = RC.device_ppo(st, replay, n_step, stride)
    assert rows == len(st.exps) == replay.cumulative_collected_count and double.record_launches == steps
    RC.assert_ring_equals(replay, st.fields, 4096 + 3)


def test_ppo_ring_wrap_pops_what_the_host_fifo_pops(double):
    RC.check_ring_wrap()


@pytest.mark.parametrize('n_step', [1, 3, 5])
def test_ddpg_transitions_equal_n_host_wrappers(double, n_step):
    n, D, A, steps, gamma = 5, 7, 3, 60, 0.99
    st = RC.host_ddpg(n, D, A, DDPG_LENGTHS, steps, n_step, gamma)
    replay = RC.uniform(D, A, n, n_step, gamma, 17)
    rec, rows = RC.device_ddpg(st, replay, n_step, gamma)
    assert rows == len(st.exps) > 17                                        # the ring of 17 wrapped
    # an episode of T steps emits max(T - n_step + 1, 0) transitions: the short ones nothing
    finished = sum(max(T - n_step + 1, 0) for m in st.monitors for T in m.episode_steps)
    assert finished <= rows <= finished + n * 14
    RC.assert_ring_equals(replay, st.fields, 17)


def test_done_step_restarts_the_clock_and_resumes_from_a_state_dict(double):
    n, D, A, n_step, stride, steps = 5, 7, 3, 4, 3, 60
    st = RC.host_ppo(n, D, A, LENGTHS, steps, n_step, stride, rnn_hidden=6)
    replay = RC.fifo(D, A, n_step, stride, 4096, rnn_hidden=6)
    checked = {'done': 0}
    holder = {}

    def check(step, rows):
        rec = holder.get('rec')
        if rec is None:
            return
        d = st.dones[step]
        want = np.where(d[:, None], st.obs_reset[step], st.obs_next[step])
        assert torch.equal(rec.observation.cpu(), torch.as_tensor(want)), step
        assert np.array_equal(rec.t[d], np.zeros(d.sum(), np.int32))
        checked['done'] += int(d.sum())
    from surreal_amd.env import DeviceWindowRecorder
    rec = DeviceWindowRecorder(n, D, A, n_step, stride, rnn_hidden=6)
    rec.begin(st.first)
    holder['rec'] = rec
    for s in range(steps):
        rec.record(replay, RC._dev(st.actions[s]), RC._dev(st.pds[s]), st.rewards[s], st.dones[s], st.obs_next[s],
                   st.obs_reset[s], cells_before=(RC._dev(st.h[s]), RC._dev(st.c[s])))
        check(s, None)
    assert checked['done'] > 10
    RC.assert_ring_equals(replay, st.fields, 4096 + 3)            # the closing windows hold the TERMINAL observations
    resumed = RC.fifo(D, A, n_step, stride, 4096, rnn_hidden=6)
    rec2, rows = RC.device_ppo(st, resumed, n_step, stride, resume_at=(7, 8, 31))
    assert rows == len(st.exps)
    RC.assert_ring_equals(resumed, st.fields, 4096 + 3)
    for k, v in rec.state_dict()['carry'].items():
        assert torch.equal(v, rec2.state_dict()['carry'][k]), k
    # and the DDPG recorder
    sd = RC.host_ddpg(n, D, A, DDPG_LENGTHS, steps, 3, 0.99)
    replay = RC.uniform(D, A, n, 3, 0.99, 4096)
    RC.device_ddpg(sd, replay, 3, 0.99, resume_at=(5, 40))
    RC.assert_ring_equals(replay, sd.fields, 4096)


def test_device_tensors_are_taken_where_host_arrays_are(double):
    n, D, A, n_step, stride, steps = 5, 8, 3, 4, 3, 30
    st = RC.host_ppo(n, D, A, LENGTHS, steps, n_step, stride)
    replay = RC.fifo(D, A, n_step, stride, 4096)
    RC.device_ppo(st, replay, n_step, stride, as_tensors=True)
    RC.assert_ring_equals(replay, st.fields, 4096 + 3)


def test_monitor_equals_the_host_monitors(double):
    from surreal_amd.env import DeviceEpisodeMonitor
    n, D, A, steps = 5, 7, 3, 60
    st = RC.host_ppo(n, D, A, LENGTHS, steps, 4, 3)
    mon = DeviceEpisodeMonitor(n, 32, 'cpu')
    RC.device_ppo(st, RC.fifo(D, A, 4, 3, 4096), 4, 3, monitor=mon)
    RC.assert_monitor_equals_host(mon, st)
    assert mon.total_steps == n * steps
    sd = RC.host_ddpg(n, D, A, DDPG_LENGTHS, steps, 3, 0.99)
    mon = DeviceEpisodeMonitor(n, 32, 'cpu')
    RC.device_ddpg(sd, RC.uniform(D, A, n, 3, 0.99, 4096), 3, 0.99, monitor=mon)
    RC.assert_monitor_equals_host(mon, sd)


# ---- the host arithmetic ---------------------------------------------------------------------------------------------
def test_ranks_and_row_counts_against_brute_force(double):
    from surreal_amd.env import DeviceWindowRecorder, DeviceNStepRecorder, closing_ranks
    rs = np.random.RandomState(11)
    for trial in range(500):
        n = int(rs.randint(1, 40))
        closes = rs.rand(n) < rs.rand()
        rank, rows = closing_ranks(closes)
        want, count = RC.brute_force_ranks(closes)
        assert rank.dtype == np.int32 and rank.tolist() == want and rows == count
    # the clocks under random done patterns: who closes, step by step, against the wrappers' conditions
    n, N, stride = 9, 4, 3
    w, d = DeviceWindowRecorder(n, 2, 1, N, stride), DeviceNStepRecorder(n, 2, 1, N, 0.9)
    t = np.zeros(n, dtype=np.int64)
    for step in range(500):
        assert w._closes(w.t).tolist() == [bool(x + 1 - N >= 0 and (x + 1 - N) % 3 == 0) for x in t]
        assert d._closes(d.t).tolist() == [bool(x >= N - 1) for x in t]
        dones = rs.rand(n) < 0.15
        w._advance(dones)
        d._advance(dones)
        t = np.where(dones, 0, t + 1)
        assert w.t.tolist() == d.t.tolist() == t.tolist()


# ---- the refusals ----------------------------------------------------------------------------------------------------
def test_recorder_refusals(double):
    from surreal_amd.env import DeviceWindowRecorder, DeviceNStepRecorder
    n, D, A = 5, 7, 3
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    rec = DeviceWindowRecorder(n, D, A, 4, 3)
    rec.begin(np.zeros((n, D), np.float32))
    replay = RC.fifo(D, A, 4, 3, 64)
    dones = np.zeros(n, bool)
    dones[2] = True
    with pytest.raises(ValueError, match='obs_reset'):
        rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), dones, np.zeros((n, D)))
    assert rec.t.tolist() == [0] * n and replay.cumulative_collected_count == 0     # nothing moved
    with pytest.raises(ValueError):                                                  # wrong shapes
        rec.record(replay, z(n, A + 1), z(n, 2 * A), np.zeros(n), np.zeros(n, bool), np.zeros((n, D)))
    with pytest.raises(ValueError):
        rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), np.zeros(n, bool), np.zeros((n, D + 1)))
    with pytest.raises(ValueError):
        rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n + 1), np.zeros(n, bool), np.zeros((n, D)))
    with pytest.raises(ValueError, match='cells_before'):
        rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), np.zeros(n, bool), np.zeros((n, D)),
                   cells_before=(z(n, 6), z(n, 6)))
    with pytest.raises(ValueError):
        rec.begin(np.zeros((n + 1, D), np.float32))
    assert rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), np.zeros(n, bool), np.zeros((n, D))) == 0
    assert rec.t.tolist() == [1] * n
    with pytest.raises(ValueError):                                                  # a table of another n_step
        DeviceWindowRecorder(n, D, A, 5, 3).record(replay, z(n, A), z(n, 2 * A), np.zeros(n), np.zeros(n, bool),
                                                   np.zeros((n, D)))
    small = RC.fifo(D, A, 4, 3, 1)                                                   # capacity 4 < 5 actors
    with pytest.raises(ValueError, match='exceed'):
        rec.record(small, z(n, A), z(n, 2 * A), np.zeros(n), np.zeros(n, bool), np.zeros((n, D)))
    drec = DeviceNStepRecorder(n, D, A, 3, 0.99)
    with pytest.raises(ValueError, match='exceed'):
        drec.record(RC.uniform(D, A, n, 3, 0.99, 4), z(n, A), np.zeros(n), np.zeros(n, bool), np.zeros((n, D)))
    with pytest.raises(ValueError):
        DeviceWindowRecorder(n, D, A, 4, 0)
    with pytest.raises(ValueError):
        DeviceNStepRecorder(0, D, A, 3, 0.99)
    with pytest.raises(ValueError):
        rec.load_state_dict(drec.state_dict())


# ---- HostVecEnv ------------------------------------------------------------------------------------------------------
def test_host_vec_env_steps_in_actor_order_and_resets_the_done(double):
    from surreal_amd.env import HostVecEnv
    n, D, A = 4, 7, 3
    log = []
    envs = [RC.ScriptedEnv(50 + a, [2, 3], D, rotation=a, log=log, tag=a) for a in range(n)]
    twins = [RC.ScriptedEnv(50 + a, [2, 3], D, rotation=a) for a in range(n)]
    venv = HostVecEnv(envs)
    first = venv.reset()
    assert first.shape == (n, D) and venv.obs_dim == D
    assert np.array_equal(first, np.stack([RC.flat(t.reset()[0]) for t in twins]))
    assert log == [(a, 'reset') for a in range(n)]
    for step in range(7):
        del log[:]
        actions = torch.full((n, A), float(step)) + torch.arange(n).view(n, 1)
        obs_next, rewards, dones, obs_reset = venv.step(actions)
        want_log = []
        for a, t in enumerate(twins):
            o, r, d, _ = t.step(None)
            want_log.append((a, 'step'))
            assert np.array_equal(obs_next[a], RC.flat(o)) and rewards[a] == np.float32(r) and dones[a] == d
            assert np.array_equal(envs[a].actions[-1], actions[a].numpy())
            if d:
                want_log.append((a, 'reset'))
                assert np.array_equal(obs_reset[a], RC.flat(t.reset()[0]))
        assert log == want_log                         # actor order, a done environment reset before the next one steps
        assert dones.tolist() == [e.t == 0 for e in envs]
    with pytest.raises(ValueError):
        HostVecEnv([])


def test_run_loops_feed_the_recorders(double):
    """run_ppo / run_ddpg with scripted agents: act on the recorder's observation, step, record, reset_batch(mask)"""
    from surreal_amd.env import HostVecEnv, DeviceWindowRecorder, DeviceNStepRecorder
    import types
    n, D, A, N, stride, T = 5, 7, 3, 4, 3, 40

    class Agent(object):
        rnn_config = types.SimpleNamespace(if_rnn_policy=False)

        def __init__(self):
            self.seen, self.masks = [], []

        def act_batch(self, obs, sigmas=None):
            self.seen.append(obs.clone())
            a = torch.tanh(obs[:, :A] + len(self.seen))
            return (a, torch.cat([a, a * 0.5], 1)) if self.ppo else a

        def reset_batch(self, mask):
            self.masks.append(mask.clone())

    for ppo in (True, False):
        agent = Agent()
        agent.ppo = ppo
        envs = [RC.ScriptedEnv(70 + a, LENGTHS, D, rotation=a) for a in range(n)]
        venv = HostVecEnv(envs)
        if ppo:
            rec, replay = DeviceWindowRecorder(n, D, A, N, stride), RC.fifo(D, A, N, stride, 4096)
            rows = venv.run_ppo(agent, rec, replay, T // 2) + venv.run_ppo(agent, rec, replay, T // 2)
        else:
            rec, replay = DeviceNStepRecorder(n, D, A, N, 0.99), RC.uniform(D, A, n, N, 0.99, 4096)
            rows = venv.run_ddpg(agent, rec, replay, T // 2) + venv.run_ddpg(agent, rec, replay, T // 2)
        assert len(agent.seen) == T and rows == replay.cumulative_collected_count > 0
        # what the agent saw: the first observations, then next / reset observations of the same scripted stream
        twins = [RC.ScriptedEnv(70 + a, LENGTHS, D, rotation=a) for a in range(n)]
        obs = np.stack([RC.flat(t.reset()[0]) for t in twins])
        dones_seen = 0
        for s in range(T):
            assert np.array_equal(agent.seen[s].numpy(), obs), (ppo, s)
            for a, t in enumerate(twins):
                o, _, d, _ = t.step(None)
                obs[a] = RC.flat(t.reset()[0]) if d else RC.flat(o)
                dones_seen += d
        assert sum(int(m.sum()) for m in agent.masks) == dones_seen > 5


# ---- the C entry points: layout and refusals before any launch ----------------------------------------------------------
@pytest.mark.parametrize('cname,pyname', [('struct smx_record_ppo_window_step', 'RecordPpoWindowStep'),
                                          ('struct smx_record_ddpg_nstep_step', 'RecordDdpgNstepStep')])
def test_record_structs_match_the_ctypes_mirrors(tmp_path, cname, pyname):
    from surreal_amd import _lib as L
    cls = getattr(L, pyname)
    got = _offsets(tmp_path, cname, cls)
    assert got['sizeof'] == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname
    assert cls._fields_[-1][0] == 'mon'


def _c_args(cls, n=5, capacity=64, rows=2, clocks=(0, 3, 4, 7, 1), ranks=(-1, 0, -1, 1, -1), **change):
    """an argument block whose device pointers are never dereferenced: every call below is refused on the host"""
    p = cls()
    fake = ctypes.c_void_p(4096)
    for name, ctype in cls._fields_:
        if ctype is ctypes.c_void_p and name not in ('t_host', 'rank_host', 'h_before', 'c_before', 'carry_cells', 'cells'):
            setattr(p, name, fake)
    p.n, p.D, p.A, p.n_step, p.rows, p.cursor, p.capacity = n, 7, 3, 4, rows, 0, capacity
    if hasattr(p, 'advance'):
        p.advance = 3
    keep = [np.asarray(clocks, dtype=np.int32), np.asarray(ranks, dtype=np.int32)]
    p.t_host, p.rank_host = (ctypes.c_void_p(x.ctypes.data) for x in keep)
    for k, v in change.items():
        setattr(p, k, v)
    return p, keep


@pytest.mark.parametrize('entry,pyname', [('smx_record_ppo_window_step_f32', 'RecordPpoWindowStep'),
                                          ('smx_record_ddpg_nstep_step_f32', 'RecordDdpgNstepStep')])
def test_c_entry_points_refuse_before_any_launch(entry, pyname):
    from surreal_amd import _lib as L
    fn, cls = getattr(L.load(), entry), getattr(L, pyname)
    assert fn(None, None) == SMX_E_NULL
    for f in ('t', 'rank', 'cur_obs', 'step_obs_next', 'step_dones', 'carry_obs', 'carry_rew', 'obs', 'obs_next', 'dones'):
        p, keep = _c_args(cls, **{f: None})
        assert fn(ctypes.byref(p), None) == SMX_E_NULL, f
    for change in (dict(n=65), dict(n=0), dict(D=0), dict(A=0), dict(n_step=0), dict(capacity=0), dict(cursor=64),
                   dict(cursor=-1), dict(rows=6), dict(rows=-1),
                   dict(rows=3),                                  # three rows reserved, two actors close
                   dict(clocks=(0, 3, -1, 7, 1)),                      # a clock before its episode
                   dict(ranks=(-1, 0, -1, 5, -1)),                 # rank >= n
                   dict(ranks=(-1, 0, -2, 1, -1))):
        p, keep = _c_args(cls, **change)
        assert fn(ctypes.byref(p), None) == SMX_E_SHAPE, change
    mon = L.EpisodeMonitor()
    mon.ep_reward = ctypes.c_void_p(4096)
    p, keep = _c_args(cls, mon=mon)
    assert fn(ctypes.byref(p), None) == SMX_E_NULL                # a monitor: all five pointers or none
    if pyname == 'RecordPpoWindowStep':
        for change, want in ((dict(advance=0), SMX_E_SHAPE), (dict(advance=5), SMX_E_SHAPE),
                             (dict(copy_workgroups=1025), SMX_E_SHAPE), (dict(step_pds=None), SMX_E_NULL),
                             (dict(h_before=ctypes.c_void_p(4096)), SMX_E_NULL),             # h without c
                             (dict(h_before=ctypes.c_void_p(4096), c_before=ctypes.c_void_p(4096)), SMX_E_NULL),  # no ring
                             (dict(carry_cells=ctypes.c_void_p(4096)), SMX_E_SHAPE)):        # a ring of 0 units
            p, keep = _c_args(cls, **change)
            assert fn(ctypes.byref(p), None) == want, change
    else:
        p, keep = _c_args(cls, gpow=None)
        assert fn(ctypes.byref(p), None) == SMX_E_NULL
