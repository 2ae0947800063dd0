"""CPU tier: the device recorders with a camera on the torch-CPU double of smx_record_ppo_pixel_window_step /
smx_record_ddpg_pixel_nstep_step -- the double itself against n host chains (FrameStackWrapper + the experience
wrappers), the recorders' host logic (staging fields, frames_reset only on done steps, begin / reset / state_dict),
HostVecEnv with a camera and its refusals, pixel=None making exactly the old launches, and the argument structs and
checks of the C entry points, which refuse a bad call before any launch."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import pixel_recorder_cases as PR
import recorder_cases as RC
from helpers import _offsets

SMX_E_NULL, SMX_E_SHAPE = -1, -2
RC_LENGTHS = [2, 4, 9, 5, 14]


@pytest.fixture
def double():
    from surreal_amd import kernels as KN
    K = PR.PixelRecorderCpuKernels()
    prev = KN.set_default_kernels(K, 'cpu')
    yield K
    KN.set_default_kernels(*prev)


# ---- the double against the host chains --------------------------------------------------------------------------------
@pytest.mark.parametrize('pixel,S,n_step,stride,Hl', [((1, 4, 4), 1, 4, 3, 0), ((3, 5, 3), 2, 4, 6, 6),
                                                      ((2, 4, 6), 3, 4, 3, 0), ((1, 4, 4), 3, 1, 1, 6)])
def test_ppo_windows_equal_n_host_chains(double, pixel, S, n_step, stride, Hl):
    n, D, A, steps = 5, 7, 3, 60
    st = PR.host_ppo_pixel(n, D, A, pixel, S, PR.LENGTHS, steps, n_step, stride, rnn_hidden=Hl)
    assert len(st.exps) > 20 and len({m.num_episodes for m in st.monitors}) > 1          # the clocks diverged
    replay = PR.fifo(D, A, n_step, stride, 4096, rnn_hidden=Hl)
    rec, rows = PR.device_ppo_pixel(st, replay, n_step, stride)
    assert rows == len(st.exps) == replay.cumulative_collected_count
    assert double.pixel_launches == double.record_launches == steps
    PR.assert_ring_equals(replay, st.fields, 4096 + 3)


@pytest.mark.parametrize('pixel,S,n_step', [((1, 4, 4), 1, 1), ((3, 5, 3), 2, 3), ((2, 4, 6), 3, 5)])
def test_ddpg_transitions_equal_n_host_chains(double, pixel, S, n_step):
    n, D, A, steps, gamma = 5, 7, 3, 60, 0.99
    st = PR.host_ddpg_pixel(n, D, A, pixel, S, PR.DDPG_LENGTHS, steps, n_step, gamma)
    replay = RC.uniform(D, A, n, n_step, gamma, 17)
    rec, rows = PR.device_ddpg_pixel(st, replay, n_step, gamma)
    assert rows == len(st.exps) > 17                                        # the ring of 17 wrapped
    PR.assert_ring_equals(replay, st.fields, 17)


def test_resumed_recorders_leave_the_same_ring(double):
    n, D, A, pixel, S, n_step, stride, steps = 5, 7, 3, (3, 5, 3), 3, 4, 3, 60
    st = PR.host_ppo_pixel(n, D, A, pixel, S, PR.LENGTHS, steps, n_step, stride, rnn_hidden=6)
    through, resumed = (PR.fifo(D, A, n_step, stride, 4096, rnn_hidden=6) for _ in range(2))
    rec, _ = PR.device_ppo_pixel(st, through, n_step, stride)
    rec2, rows = PR.device_ppo_pixel(st, resumed, n_step, stride, resume_at=(1, 7, 8, 31))
    assert rows == len(st.exps)
    PR.assert_ring_equals(resumed, st.fields, 4096 + 3)
    a, b = rec.state_dict(), rec2.state_dict()
    assert a['hist_pos'] == b['hist_pos'] == steps % (n_step + S)
    for k in ('hist', 'obs_pixel', 'cur_obs'):
        assert torch.equal(a[k], b[k]), k
    sd = PR.host_ddpg_pixel(n, D, A, pixel, S, PR.DDPG_LENGTHS, steps, 3, 0.99)
    replay = RC.uniform(D, A, n, 3, 0.99, 4096)
    PR.device_ddpg_pixel(sd, replay, 3, 0.99, resume_at=(5, 40))
    PR.assert_ring_equals(replay, sd.fields, 4096)


# ---- the recorders' host logic -----------------------------------------------------------------------------------------
def test_staging_fields_and_frames_reset_only_on_done_steps(double):
    from surreal_amd.env import DeviceWindowRecorder
    from surreal_amd.env.device_recorder import _StagingSet
    n, D, A, pixel, S = 5, 7, 3, (3, 5, 3), 2
    F = 45
    s = _StagingSet(n, D, torch.device('cpu'), F)
    assert s.fields == ('t', 'rank', 'dones', 'rewards', 'obs_next', 'obs_reset', 'frames_next', 'frames_reset')
    assert _StagingSet(n, D, torch.device('cpu')).fields == _StagingSet.FIELDS           # no camera: the old set
    assert _StagingSet(n, D, torch.device('cpu')).host.numel() == 4 * 8 + 2 * 36
    for k in ('frames_next', 'frames_reset'):
        assert s.h[k].dtype == np.uint8 and s.h[k].shape == (n, F) and s.d[k].dtype == torch.uint8
        assert s.d[k].shape == (n, F) and s.h[k].ctypes.data % 16 == 0
    assert s.end['frames_reset'] == s.host.numel() and s.end['frames_next'] + 60 == s.end['frames_reset']
    # what travels: one copy per step, up to frames_next; up to frames_reset only where some actor is done
    uploads = []
    rec = DeviceWindowRecorder(n, D, A, 4, 3, pixel=pixel, frame_stacks=S)
    for st_ in rec._sets:
        st_.upload = (lambda last, st_=st_: uploads.append(last))
    rec.begin(np.zeros((n, D), np.float32), np.zeros((n,) + pixel, np.uint8))
    replay = PR.fifo(D, A, 4, 3, 64)
    z = lambda *sh: torch.zeros(*sh)  # noqa: E731
    fr = np.full((n,) + pixel, 7, np.uint8)
    seen = []
    orig = double.record_ppo_pixel_window_step
    double.record_ppo_pixel_window_step = lambda r, **kw: (seen.append(r.get('frames_reset')), orig(r, **kw))
    dones = np.zeros(n, bool)
    rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), dones, np.zeros((n, D)), np.zeros((n, D)), frames_next=fr,
               frames_reset=fr)
    assert uploads == ['frames_next'] and seen == [None]
    dones[3] = True
    rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), dones, np.zeros((n, D)), np.zeros((n, D)), frames_next=fr,
               frames_reset=fr)
    assert uploads == ['frames_next', 'frames_reset'] and seen[1] is not None
    assert rec.t.tolist() == [2, 2, 2, 0, 2] and rec.hist_pos == 2
    with pytest.raises(ValueError, match='frames_reset'):
        rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), dones, np.zeros((n, D)), np.zeros((n, D)), frames_next=fr)
    with pytest.raises(ValueError, match='frames_next'):
        rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), ~dones & False, np.zeros((n, D)))
    with pytest.raises(ValueError, match='uint8'):
        rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), ~dones & False, np.zeros((n, D)),
                   frames_next=fr.astype(np.float32))
    with pytest.raises(ValueError, match='uint8'):
        rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), ~dones & False, np.zeros((n, D)), frames_next=fr[:, :2])
    assert rec.t.tolist() == [2, 2, 2, 0, 2] and rec.hist_pos == 2 and len(uploads) == 2           # nothing moved


def test_begin_reset_and_state_dict(double):
    from surreal_amd.env import DeviceWindowRecorder, DeviceNStepRecorder
    n, D, A, pixel, S, N = 4, 7, 3, (2, 4, 6), 3, 4
    rs = np.random.RandomState(5)
    frames = lambda: rs.randint(0, 256, (n,) + pixel).astype(np.uint8)  # noqa: E731
    rec = DeviceWindowRecorder(n, D, A, N, 3, pixel=pixel, frame_stacks=S)
    assert tuple(rec.hist.shape) == (n, N + S) + pixel and rec.hist.dtype == torch.uint8
    assert rec.shapes['pixel'] == (N, 6, 4, 6) and rec.shapes['pixel_next'] == (1, 6, 4, 6)
    assert DeviceNStepRecorder(n, D, A, N, 0.9, pixel=pixel, frame_stacks=S).shapes['pixel'] == (6, 4, 6)
    f0, o0 = frames(), rs.standard_normal((n, D)).astype(np.float32)
    rec.begin(o0, f0)
    obs = rec.observation
    assert isinstance(obs, collections.OrderedDict) and tuple(obs['pixel']['camera0'].shape) == (n, 6, 4, 6)
    assert np.array_equal(obs['pixel']['camera0'].numpy(), np.tile(f0, (1, S, 1, 1)))
    assert np.array_equal(rec.hist[:, 0].numpy(), f0) and rec.hist_pos == 0
    assert np.array_equal(obs['low_dim']['flat_inputs'].numpy(), o0)
    # a few steps, then reset two actors outside record()
    replay = PR.fifo(D, A, N, 3, 64)
    z = lambda *sh: torch.zeros(*sh)  # noqa: E731
    for _ in range(3):
        rec.record(replay, z(n, A), z(n, 2 * A), np.zeros(n), np.zeros(n, bool), o0, frames_next=frames())
    before = rec.obs_pixel.clone()
    mask = np.array([False, True, False, True])
    f1, o1 = frames(), rs.standard_normal((n, D)).astype(np.float32)
    rec.reset(mask, o1, f1)
    assert rec.t.tolist() == [3, 0, 3, 0] and rec.hist_pos == 3
    assert np.array_equal(rec.obs_pixel[mask].numpy(), np.tile(f1[mask], (1, S, 1, 1)))
    assert torch.equal(rec.obs_pixel[~mask], before[~mask])
    assert np.array_equal(rec.hist[mask, 3].numpy(), f1[mask])
    assert np.array_equal(rec.cur_obs.numpy(), np.where(mask[:, None], o1, o0))
    with pytest.raises(ValueError, match='together'):
        rec.reset(mask, o1)
    with pytest.raises(ValueError, match='frames'):
        rec.begin(o0)
    with pytest.raises(ValueError, match='uint8'):
        rec.begin(o0, f0.astype(np.int32))
    # state_dict carries hist, hist_pos and the acting observation; a recorder without a camera refuses it
    sd = rec.state_dict()
    assert sd['hist_pos'] == 3 and torch.equal(sd['hist'], rec.hist) and torch.equal(sd['obs_pixel'], rec.obs_pixel)
    twin = DeviceWindowRecorder(n, D, A, N, 3, pixel=pixel, frame_stacks=S)
    twin.load_state_dict(sd)
    assert twin.hist_pos == 3 and torch.equal(twin.hist, rec.hist) and torch.equal(twin.obs_pixel, rec.obs_pixel)
    assert twin.t.tolist() == rec.t.tolist()
    with pytest.raises(ValueError, match='camera'):
        DeviceWindowRecorder(n, D, A, N, 3).load_state_dict(sd)
    with pytest.raises(ValueError, match='camera'):
        twin.load_state_dict(DeviceWindowRecorder(n, D, A, N, 3).state_dict())
    with pytest.raises(ValueError):
        DeviceWindowRecorder(n, D, A, N, 3, pixel=pixel, frame_stacks=2).load_state_dict(sd)
    with pytest.raises(ValueError):
        DeviceWindowRecorder(n, D, A, N, 3, pixel=(2, 4), frame_stacks=2)
    with pytest.raises(ValueError):
        DeviceWindowRecorder(n, D, A, N, 3, pixel=pixel, frame_stacks=0)
    with pytest.raises(ValueError, match='without a camera'):
        DeviceWindowRecorder(n, D, A, N, 3).begin(o0, f0)


def test_without_a_camera_the_old_launches_are_made(double):
    """pixel=None: the same launches with the same arguments -- the double's counters, and the argument dict's keys"""
    n, D, A, n_step, stride, steps = 5, 7, 3, 4, 3, 30
    keys = []
    orig = double.record_ppo_window_step
    double.record_ppo_window_step = lambda r, **kw: (keys.append((sorted(r), sorted(kw))), orig(r, **kw))
    st = RC.host_ppo(n, D, A, RC_LENGTHS, steps, n_step, stride)
    replay = RC.fifo(D, A, n_step, stride, 4096)
    rec, rows = RC.device_ppo(st, replay, n_step, stride)
    assert double.record_launches == steps and double.pixel_launches == 0
    assert rec.pixel is None and torch.is_tensor(rec.observation) and 'hist' not in rec.state_dict()
    assert all(k == (sorted(['t', 'rank', 'dones', 'rewards', 'obs_next', 'obs_reset', 't_host', 'rank_host', 'rows',
                             'cur_obs', 'actions', 'pds', 'h_before', 'c_before', 'n_step', 'advance', 'carry', 'tables',
                             'cursor']), ['copy_workgroups', 'monitor']) for k in keys)
    RC.assert_ring_equals(replay, st.fields, 4096 + 3)
    sd = RC.host_ddpg(n, D, A, [2, 3, 9, 5, 14], steps, 3, 0.99)
    RC.device_ddpg(sd, RC.uniform(D, A, n, 3, 0.99, 4096), 3, 0.99)
    assert double.record_launches == 2 * steps and double.pixel_launches == 0


# ---- HostVecEnv --------------------------------------------------------------------------------------------------------
def _camera_envs(n, D, pixel, lengths=(2, 3), seed=50):
    return [PR.ScriptedCameraEnv(seed + a, lengths, D, pixel, rotation=a) for a in range(n)]


def test_host_vec_env_returns_the_raw_frames(double):
    from surreal_amd.env import HostVecEnv
    n, D, A, pixel = 4, 7, 3, (3, 5, 3)
    venv = HostVecEnv(_camera_envs(n, D, pixel), frame_stacks=2)
    twins = _camera_envs(n, D, pixel)
    obs, frames = venv.reset()
    assert venv.obs_dim == D and venv.pixel == pixel and frames.dtype == np.uint8 and frames.shape == (n,) + pixel
    first = [t.reset()[0] for t in twins]
    assert np.array_equal(obs, np.stack([RC.flat(o) for o in first]))
    assert np.array_equal(frames, np.stack([PR.cam(o) for o in first]))
    for step in range(7):
        obs_next, rewards, dones, obs_reset, f_next, f_reset = venv.step(torch.zeros(n, A))
        for a, t in enumerate(twins):
            o, r, d, _ = t.step(None)
            assert np.array_equal(obs_next[a], RC.flat(o)) and np.array_equal(f_next[a], PR.cam(o)) and dones[a] == d
            if d:
                o = t.reset()[0]
                assert np.array_equal(obs_reset[a], RC.flat(o)) and np.array_equal(f_reset[a], PR.cam(o))


def test_host_vec_env_refusals(double):
    from surreal_amd.env import HostVecEnv, DeviceWindowRecorder
    import types
    n, D, A, pixel, S = 3, 7, 3, (1, 4, 4), 2

    def env_with(change):
        env = PR.ScriptedCameraEnv(1, [3], D, pixel)
        plain = env._observe
        env._observe = lambda: change(plain())
        return env

    def drop_camera(obs):
        del obs['pixel']
        return obs

    def second_camera(obs):
        obs['pixel']['camera1'] = obs['pixel']['camera0']
        return obs

    def pixel_only(obs):
        obs['low_dim'] = collections.OrderedDict()
        return obs

    def stacked_on_host(obs):
        obs['pixel']['camera0'] = [obs['pixel']['camera0']] * 2
        return obs
    good = lambda: PR.ScriptedCameraEnv(2, [3], D, pixel)  # noqa: E731
    for change, why in ((drop_camera, 'only some'), (second_camera, 'one camera'), (pixel_only, 'pixel-only'),
                        (stacked_on_host, 'stacked on the host')):
        with pytest.raises(ValueError, match=why):
            HostVecEnv([good(), env_with(change)], frame_stacks=S).reset()
    with pytest.raises(ValueError, match='only some'):                       # ... also when it shows on a later step
        venv = HostVecEnv([good(), good()], frame_stacks=S)
        venv.reset()
        venv.envs[1]._observe = lambda: drop_camera(PR.ScriptedCameraEnv._observe(venv.envs[1]))
        venv.step(torch.zeros(2, A))
    with pytest.raises(ValueError):                                          # a camera nobody asked for
        HostVecEnv([good()]).reset()
    with pytest.raises(ValueError):
        HostVecEnv([good()], frame_stacks=0)
    # the agent's camera0 must be the stacked frame; the recorder's camera the environments'
    agent = types.SimpleNamespace(rnn_config=types.SimpleNamespace(if_rnn_policy=False),
                                  obs_spec={'pixel': {'camera0': (3 * pixel[0],) + pixel[1:]}, 'low_dim': {'flat_inputs': (D,)}})
    venv = HostVecEnv([good() for _ in range(n)], frame_stacks=S)
    rec = DeviceWindowRecorder(n, D, A, 4, 3, pixel=pixel, frame_stacks=S)
    with pytest.raises(ValueError, match='camera0'):
        venv.run_ppo(agent, rec, PR.fifo(D, A, 4, 3, 64), 1)
    with pytest.raises(ValueError, match='camera0'):
        venv.run_ddpg(agent, rec, None, 1)
    with pytest.raises(ValueError, match='recorder'):
        venv.run_ppo(agent, DeviceWindowRecorder(n, D, A, 4, 3), PR.fifo(D, A, 4, 3, 64), 1)
    with pytest.raises(ValueError, match='recorder'):
        venv.run_ppo(agent, DeviceWindowRecorder(n, D, A, 4, 3, pixel=pixel, frame_stacks=3), None, 1)


def test_run_loops_feed_the_camera_recorders(double):
    """run_ppo / run_ddpg with a scripted camera agent: it acts on the nested observation, whose camera0 is the stack a
    host FrameStackWrapper chain would show it"""
    from surreal_amd.env import HostVecEnv, DeviceWindowRecorder, DeviceNStepRecorder, FrameStackWrapper
    from surreal_amd.session import Config
    import types
    n, D, A, pixel, S, N, stride, T = 5, 7, 3, (3, 5, 3), 2, 4, 3, 40

    class Agent(object):
        rnn_config = types.SimpleNamespace(if_rnn_policy=False)
        obs_spec = {'pixel': {'camera0': (S * pixel[0],) + pixel[1:]}, 'low_dim': {'flat_inputs': (D,)}}

        def __init__(self, ppo):
            self.ppo, self.seen = ppo, []

        def act_batch(self, obs, sigmas=None):
            self.seen.append(obs['pixel']['camera0'].clone())
            a = torch.tanh(obs['low_dim']['flat_inputs'][:, :A])
            return (a, torch.cat([a, a * 0.5], 1)) if self.ppo else a

        def reset_batch(self, mask):
            pass

    for ppo in (True, False):
        agent = Agent(ppo)
        venv = HostVecEnv(_camera_envs(n, D, pixel, PR.LENGTHS, 70), frame_stacks=S)
        if ppo:
            rec = DeviceWindowRecorder(n, D, A, N, stride, pixel=pixel, frame_stacks=S)
            replay = PR.fifo(D, A, N, stride, 4096)
            rows = venv.run_ppo(agent, rec, replay, T // 2) + venv.run_ppo(agent, rec, replay, T // 2)
        else:
            rec = DeviceNStepRecorder(n, D, A, N, 0.99, pixel=pixel, frame_stacks=S)
            replay = RC.uniform(D, A, n, N, 0.99, 4096)
            rows = venv.run_ddpg(agent, rec, replay, T // 2) + venv.run_ddpg(agent, rec, replay, T // 2)
        assert len(agent.seen) == T and rows == replay.cumulative_collected_count > 0
        chains = [FrameStackWrapper(e, Config(frame_stacks=S, frame_stack_concatenate_on_env=True))
                  for e in _camera_envs(n, D, pixel, PR.LENGTHS, 70)]
        obs = [c.reset()[0] for c in chains]
        for s in range(T):
            assert np.array_equal(agent.seen[s].numpy(), np.stack([PR.cam(o) for o in obs])), (ppo, s)
            for a, c in enumerate(chains):
                o, _, d, _ = c.step(None)
                obs[a] = c.reset()[0] if d else o
        f = replay.sample_batch(8)
        batch = venv.to_batch(f) if ppo else venv.to_ddpg_batch(f)
        assert list(batch['obs']) == ['low_dim', 'pixel'] and batch['obs']['pixel']['camera0'].dtype == torch.uint8
        assert batch['obs_next']['pixel']['camera0'] is f['pixel_next']
        if not ppo:
            assert tuple(batch['rewards'].shape) == (8, 1) and tuple(batch['dones'].shape) == (8, 1)
            assert tuple(batch['obs']['pixel']['camera0'].shape) == (8, S * pixel[0]) + pixel[1:]


# ---- the C entry points: layout and refusals before any launch ----------------------------------------------------------
@pytest.mark.parametrize('cname,pyname', [('struct smx_record_ppo_pixel_window_step', 'RecordPpoPixelWindowStep'),
                                          ('struct smx_record_ddpg_pixel_nstep_step', 'RecordDdpgPixelNstepStep')])
def test_pixel_record_structs_match_the_ctypes_mirrors(tmp_path, cname, pyname):
    from surreal_amd import _lib as L
    cls = getattr(L, pyname)
    got = _offsets(tmp_path, cname, cls)
    assert got['sizeof'] == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname
    assert cls._fields_[-1][0] == 'mon' and len({f for f, _ in cls._fields_}) == len(cls._fields_)


def c_args(cls, n=5, capacity=64, rows=2, clocks=(0, 3, 4, 7, 1), ranks=(-1, 0, -1, 1, -1), **change):
    """an argument block whose device pointers are never dereferenced: every call below is refused on the host
    (n_step 4, advance 3, frame_stacks 3, hist_len 7: the minimum)"""
    p = cls()
    fake = ctypes.c_void_p(4096)
    for name, ctype in cls._fields_:
        if ctype is ctypes.c_void_p and name not in ('t_host', 'rank_host', 'h_before', 'c_before', 'carry_cells', 'cells'):
            setattr(p, name, fake)
    p.n, p.D, p.A, p.n_step, p.rows, p.cursor, p.capacity = n, 7, 3, 4, rows, 0, capacity
    p.C, p.H, p.W, p.frame_stacks, p.hist_len, p.hist_pos = 1, 4, 4, 3, 7, 6
    if hasattr(p, 'advance'):
        p.advance = 3
    keep = [np.asarray(clocks, dtype=np.int32), np.asarray(ranks, dtype=np.int32)]
    p.t_host, p.rank_host = (ctypes.c_void_p(x.ctypes.data) for x in keep)
    for k, v in change.items():
        setattr(p, k, v)
    return p, keep


ENTRIES = [('smx_record_ppo_pixel_window_step', 'RecordPpoPixelWindowStep'),
           ('smx_record_ddpg_pixel_nstep_step', 'RecordDdpgPixelNstepStep')]
BAD_SHAPES = (dict(hist_len=6),                                # < n_step + frame_stacks
              dict(hist_pos=7), dict(hist_pos=-1),             # outside the history
              dict(n=65), dict(D=0), dict(C=0), dict(W=0), dict(frame_stacks=0), dict(copy_workgroups=1025),
              dict(rows=3),                                    # three rows reserved, two actors close
              dict(clocks=(0, 3, -1, 7, 1)), dict(ranks=(-1, 0, -1, 5, -1)))


@pytest.mark.parametrize('entry,pyname', ENTRIES)
def test_c_entry_points_refuse_before_any_launch(entry, pyname):
    from surreal_amd import _lib as L
    fn, cls = getattr(L.load(), entry), getattr(L, pyname)
    assert fn(None, None) == SMX_E_NULL
    for f in ('t', 'cur_obs', 'carry_obs', 'obs', 'hist', 'pixel', 'pixel_next', 'obs_pixel', 'step_frame_next'):
        p, keep = c_args(cls, **{f: None})
        assert fn(ctypes.byref(p), None) == SMX_E_NULL, f
    for change in BAD_SHAPES:
        p, keep = c_args(cls, **change)
        assert fn(ctypes.byref(p), None) == SMX_E_SHAPE, change
