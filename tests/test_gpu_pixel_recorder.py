"""GPU tier (-m gpu): the camera record launches (smx_record_ppo_pixel_window_step / smx_record_ddpg_pixel_nstep_step)
behind DeviceWindowRecorder / DeviceNStepRecorder with ``pixel=..., frame_stacks=...`` against n host chains
env -> FrameStackWrapper -> experience wrapper stepped in actor order -- byte for byte: these launches copy bytes, and
DDPG's reward is the same fp64 sum in the same order --, against the ring bytes the synthetic camera rollouts leave on
equal clocks, the host EpisodeMonitor, resumed recorders, and end to end from HostVecEnv through the replays to the
CNN-stem learners."""
import functools

import numpy as np
import pytest
import torch

import ddpg_pixel_rollout_cases as PC
import pixel_recorder_cases as PR
import ppo_pixel_window_cases as PP
import recorder_cases as RC

pytestmark = pytest.mark.gpu

N_ACTORS, D, A, STEPS = 5, 7, 3, 60
PIXELS = [(1, 4, 4), (3, 5, 3), (2, 4, 6)]       # F = 16: the 16-byte path; F = 45: the byte path; F = 48


@functools.lru_cache(maxsize=None)
def ppo_stream(pixel, S, n_step, stride, Hl):
    """the host chains' windows and step stream, computed once per case and left unchanged"""
    return PR.host_ppo_pixel(N_ACTORS, D, A, pixel, S, PR.LENGTHS, STEPS, n_step, stride, rnn_hidden=Hl)


@functools.lru_cache(maxsize=None)
def ddpg_stream(pixel, S, n_step):
    return PR.host_ddpg_pixel(N_ACTORS, D, A, pixel, S, PR.DDPG_LENGTHS, STEPS, n_step, 0.99)


@pytest.mark.parametrize('copy_workgroups', [0, 3])
@pytest.mark.parametrize('Hl', [0, 6])
@pytest.mark.parametrize('n_step,stride', [(4, 3), (4, 6), (1, 1)])
@pytest.mark.parametrize('S', [1, 2, 3])
@pytest.mark.parametrize('pixel', PIXELS)
def test_ppo_windows_equal_n_host_chains(pixel, S, n_step, stride, Hl, copy_workgroups):
    """episode lengths [2, 4, 9, 5, 14]: shorter than S, shorter than N, equal to N, closing on the terminal step, long;
    the history at its minimum n_step + S; the acting observation after every step is the chain's next stacked one
    (device_ppo_pixel checks it)"""
    st = ppo_stream(pixel, S, n_step, stride, Hl)
    replay = PR.fifo(D, A, n_step, stride, 4096, rnn_hidden=Hl)
    rec, rows = PR.device_ppo_pixel(st, replay, n_step, stride, copy_workgroups=copy_workgroups, hist_len=n_step + S)
    torch.cuda.synchronize()
    assert rows == len(st.exps) == replay.cumulative_collected_count > 20
    PR.assert_ring_equals(replay, st.fields, 4096 + 3)


@pytest.mark.parametrize('n_step', [1, 3, 5])
@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('pixel', PIXELS)
def test_ddpg_transitions_equal_n_host_chains(pixel, S, n_step):
    st = ddpg_stream(pixel, S, n_step)
    replay = RC.uniform(D, A, N_ACTORS, n_step, 0.99, 17)
    rec, rows = PR.device_ddpg_pixel(st, replay, n_step, 0.99, copy_workgroups=0 if S == 1 else 2)
    torch.cuda.synchronize()
    assert rows == len(st.exps) > 17                                  # the ring of 17 wrapped
    PR.assert_ring_equals(replay, st.fields, 17)


def test_device_tensors_are_taken_where_host_arrays_are():
    st = ppo_stream((1, 4, 4), 2, 4, 3, 0)
    replay = PR.fifo(D, A, 4, 3, 4096)
    PR.device_ppo_pixel(st, replay, 4, 3, as_tensors=True)
    PR.assert_ring_equals(replay, st.fields, 4096 + 3)


# ---- equal clocks: the layout of the synthetic camera rollouts ---------------------------------------------------------
def _frames(K, s0, t, pixel):
    out = torch.empty((s0.shape[0],) + pixel, dtype=torch.uint8, device='cuda')
    K.synth_frames(s0.contiguous(), t, out)
    return out


def _replay_stream(rows, n, L_, T, pixel, init_state, record):
    """the per-step rows (n_step 1: row s * n + a holds actor a's step s) of a synthetic camera rollout, fed step by step
    to record(s, step fields, dones, frames_next, frames_reset); the frames made with synth_frames from the states"""
    from surreal_amd import kernels as KN
    K = KN.default_kernels()
    reset_frames = _frames(K, init_state[:, 0], 0, pixel)
    for s in range(T):
        tau = s % L_
        f = {k: v[s * n:(s + 1) * n].contiguous() for k, v in rows.items()}
        done = np.full(n, tau + 1 >= L_)
        assert bool(f['dones'].reshape(n, -1)[0, -1]) == bool(done[0])
        record(s, f, done, _frames(K, f['obs_next'].reshape(n, -1)[:, 0], tau + 1, pixel), reset_frames)


def test_equal_clocks_give_the_ppo_rollouts_ring():
    """every actor on the same clock.  The step stream of a camera SyntheticVecEnv -- its n_step-1 windows, which hold
    every step -- recorded step by step leaves the ring bytes ppo_rollout_into leaves for the same agent parameters,
    seeds and eps at (n_step, stride) = (4, 3): the layout the learners are held to"""
    from surreal_amd.env import DeviceWindowRecorder
    from surreal_amd.replay import FIFOReplay
    n, Dv, Av, N, stride, L_, pixel, S = 6, 11, 3, 4, 3, 13, (3, 36, 36), 2
    T = 2 * L_ + 5
    assert (L_ - N) % 3 == 0                                          # a window closes on the terminal step
    eps = torch.randn(T, n, Av, generator=torch.Generator().manual_seed(2)).cuda()
    kw = dict(hidden=(64, 32), feat=32, memory_size=4096, final_scale=1.0)
    rings = {}
    for key, (ns, sd) in (('steps', (1, 1)), ('windows', (N, stride))):
        agent, (lc, ec, sc) = PP.make_agent(Dv, Av, ns, sd, pixel, S, **kw)
        venv = PP.make_venv(n, Dv, Av, L_, pixel, S)
        replay = FIFOReplay(lc, ec, sc)
        written = venv.ppo_rollout_into(agent, replay, T, eps=eps)
        rings[key] = ({k: t.data[:written].clone() for k, t in replay._tables.items()}, written, venv.init_state.clone())
    steps, written, init_state = rings['steps']
    assert written == n * T
    want, rows_want, _ = rings['windows']
    replay = PR.fifo(Dv, Av, N, stride, 4096)
    rec = DeviceWindowRecorder(n, Dv, Av, N, stride, pixel=pixel, frame_stacks=S)
    rec.begin(init_state, _frames(rec.K, init_state[:, 0], 0, pixel))
    got_rows = []
    _replay_stream(steps, n, L_, T, pixel, init_state, lambda s, f, done, fn, fr: got_rows.append(
        rec.record(replay, f['actions'], f['pds'], f['rewards'].reshape(n), done, f['obs_next'], init_state,
                   frames_next=fn, frames_reset=fr)))
    torch.cuda.synchronize()
    assert sum(got_rows) == rows_want > 0 and set(got_rows) == {0, n}
    assert set(want) == set(replay._tables)
    for k, w in want.items():
        assert torch.equal(replay._tables[k].data[:rows_want], w), k


def test_equal_clocks_give_the_ddpg_rollouts_ring():
    """the same for ddpg_rollout_into: the n_step-1 transitions are the step stream (their reward is the step's), the
    recorder at n_step 3 leaves the ring of the n_step-3 rollout"""
    from surreal_amd.env import DeviceNStepRecorder, SyntheticVecEnv
    from surreal_amd.replay import UniformReplay
    n, Dv, Av, N, L_, pixel, S = 6, 11, 3, 3, 9, (3, 36, 36), 2
    T = 2 * L_ + 5
    eps = torch.randn(T, n, Av, generator=torch.Generator().manual_seed(4)).cuda()
    rings = {}
    for ns in (1, N):
        lc, ec, sc = PC.configs(Dv, Av, n, pixel, S, hidden=(64, 32), feat=32, memory_size=4096, n_step=ns, gamma=0.99,
                                noise_type='normal')
        agent = PC.DC.make_agent(lc, ec, sc, w3_scale=1.0)
        venv = SyntheticVecEnv(n, Dv, Av, episode_len=L_, device='cuda', pixel=pixel, frame_stacks=S)
        replay = UniformReplay(lc, ec, sc)
        written = venv.ddpg_rollout_into(agent, replay, T, eps=eps)
        rings[ns] = ({k: t.data[:written].clone() for k, t in replay._tables.items()}, written, venv.init_state.clone())
    steps, written, init_state = rings[1]
    assert written == n * T
    want, rows_want, _ = rings[N]
    replay = RC.uniform(Dv, Av, n, N, 0.99, 4096)
    rec = DeviceNStepRecorder(n, Dv, Av, N, 0.99, pixel=pixel, frame_stacks=S)
    rec.begin(init_state, _frames(rec.K, init_state[:, 0], 0, pixel))
    total = []
    _replay_stream(steps, n, L_, T, pixel, init_state, lambda s, f, done, fn, fr: total.append(
        rec.record(replay, f['actions'], f['rewards'].reshape(n), done, f['obs_next'], init_state, frames_next=fn,
                   frames_reset=fr)))
    torch.cuda.synchronize()
    assert sum(total) == rows_want > 0
    assert set(want) == set(replay._tables)
    for k, w in want.items():
        assert torch.equal(replay._tables[k].data[:rows_want], w), k


# ---- resume, monitor ---------------------------------------------------------------------------------------------------
def test_resumed_recorders_leave_the_same_ring():
    pixel, S, n_step, stride, Hl = (3, 5, 3), 3, 4, 3, 6
    st = ppo_stream(pixel, S, n_step, stride, Hl)
    through, resumed = (PR.fifo(D, A, n_step, stride, 4096, rnn_hidden=Hl) for _ in range(2))
    rec, _ = PR.device_ppo_pixel(st, through, n_step, stride)
    rec2, rows = PR.device_ppo_pixel(st, resumed, n_step, stride, resume_at=(1, 7, 8, 31))
    torch.cuda.synchronize()
    assert rows == len(st.exps)
    PR.assert_ring_equals(resumed, st.fields, 4096 + 3)
    a, b = rec.state_dict(), rec2.state_dict()
    assert a['hist_pos'] == b['hist_pos'] and a['t'].tolist() == b['t'].tolist()
    for k in ('hist', 'obs_pixel', 'cur_obs'):
        assert torch.equal(a[k], b[k]), k
    sd = ddpg_stream(pixel, S, 3)
    replay = RC.uniform(D, A, N_ACTORS, 3, 0.99, 4096)
    PR.device_ddpg_pixel(sd, replay, 3, 0.99, resume_at=(5, 40))
    PR.assert_ring_equals(replay, sd.fields, 4096)


def test_monitor_equals_the_host_monitors():
    from surreal_amd.env import DeviceEpisodeMonitor
    st = ppo_stream((2, 4, 6), 2, 4, 3, 0)
    mon = DeviceEpisodeMonitor(N_ACTORS, 32, 'cuda')
    PR.device_ppo_pixel(st, PR.fifo(D, A, 4, 3, 4096), 4, 3, monitor=mon)
    RC.assert_monitor_equals_host(mon, st)
    assert mon.total_steps == N_ACTORS * STEPS
    sd = ddpg_stream((2, 4, 6), 3, 3)
    mon = DeviceEpisodeMonitor(N_ACTORS, 32, 'cuda')
    PR.device_ddpg_pixel(sd, RC.uniform(D, A, N_ACTORS, 3, 0.99, 4096), 3, 0.99, monitor=mon)
    RC.assert_monitor_equals_host(mon, sd)


# ---- end to end at tiny shapes -------------------------------------------------------------------------------------------
E2E_PIXEL, E2E_S = (1, 36, 36), 2


def _camera_envs(n, Dv, lengths, seed):
    return [PR.ScriptedCameraEnv(seed + a, lengths, Dv, E2E_PIXEL, rotation=a) for a in range(n)]


def test_host_vec_env_to_fifo_to_ppo_learn():
    from surreal_amd import synthetic
    from surreal_amd.env import HostVecEnv, DeviceWindowRecorder, DeviceEpisodeMonitor
    from surreal_amd.learner import PPOLearner
    from surreal_amd.replay import FIFOReplay
    n, Dv, Av, N, stride, T, B, feat = 6, 17, 6, 5, 3, 60, 64, 32
    lengths = [12, 7, 20, 9]
    agent, (lc, ec, sc) = PP.make_agent(Dv, Av, N, stride, E2E_PIXEL, E2E_S, hidden=(64, 32), feat=feat,
                                        memory_size=512, batch_size=B)
    learner = PPOLearner(lc, ec, sc)
    learner.model.load_params(synthetic.make_ppo_params(Dv, Av, hidden=(64, 32), seed=9,
                                                        pixel=(E2E_S * E2E_PIXEL[0],) + E2E_PIXEL[1:],
                                                        cnn_feature_dim=feat))
    replay = FIFOReplay(lc, ec, sc)
    venv = HostVecEnv(_camera_envs(n, Dv, lengths, 90), frame_stacks=E2E_S)
    rec = DeviceWindowRecorder(n, Dv, Av, N, stride, pixel=E2E_PIXEL, frame_stacks=E2E_S)
    mon = DeviceEpisodeMonitor(n, 32, 'cuda')
    written = venv.run_ppo(agent, rec, replay, T // 2, monitor=mon) + venv.run_ppo(agent, rec, replay, T // 2, monitor=mon)
    torch.cuda.synchronize()
    assert written == replay.cumulative_collected_count == len(replay) >= B
    mon.poll()
    assert [len(x) for x in mon.episode_steps] == [e.episode - 1 for e in venv.envs]
    views = replay.sample_batch(B, copy=False)
    assert views['pixel'].dtype == torch.uint8 and tuple(views['pixel'].shape) == (B, N, 2, 36, 36)
    stats = learner.learn(venv.to_batch(views))
    for k, v in stats.items():
        assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k
    assert len(replay) == written - B


def test_host_vec_env_to_uniform_replay_to_ddpg_learn():
    from surreal_amd.env import HostVecEnv, DeviceNStepRecorder
    from surreal_amd.learner.ddpg import DDPGLearner
    from surreal_amd.replay import UniformReplay
    n, Dv, Av, N, T, B = 6, 17, 6, 3, 40, 64
    lc, ec, sc = PC.configs(Dv, Av, n, E2E_PIXEL, E2E_S, hidden=(64, 32), feat=32, memory_size=1024, n_step=N)
    lc.replay.batch_size = B
    agent = PC.DC.make_agent(lc, ec, sc, w3_scale=1.0)
    replay = UniformReplay(lc, ec, sc)
    venv = HostVecEnv(_camera_envs(n, Dv, PR.DDPG_LENGTHS, 40), frame_stacks=E2E_S)
    rec = DeviceNStepRecorder(n, Dv, Av, N, lc.algo.gamma, pixel=E2E_PIXEL, frame_stacks=E2E_S)
    written = venv.run_ddpg(agent, rec, replay, T, sigmas=agent.batch_sigmas(n).float())
    torch.cuda.synchronize()
    assert written == replay.cumulative_collected_count == len(replay) > B
    learner = DDPGLearner(lc, ec, sc)
    f = replay.sample_batch(B, out=learner.staging_fields(B))
    assert f['pixel'].dtype == torch.uint8 and tuple(f['pixel'].shape) == (B, 2, 36, 36)
    assert (f['pixel'].reshape(B, -1).float().sum(1) > 0).all()      # every sampled row holds a transition's frames
    stats = learner.learn(venv.to_ddpg_batch(f))
    for k, v in dict(stats).items():
        assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k


# ---- bad arguments: the documented codes, nothing launched ---------------------------------------------------------------
def _launch_args(ppo, n=5, cap=8, N=4, S=3, Hd=None, pos=0, rank=(-1, 0, -1, 1, -1), rows=2):
    C, Hh, W = 1, 4, 4
    Hd = N + S if Hd is None else Hd
    dev = 'cuda'
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
    t = np.asarray([0, 3, 4, 6, 1][:n] + [0] * (n - 5), np.int32)      # actors 1 and 3 close (PPO: j = 0, 3)
    rank = np.asarray(list(rank)[:n] + [-1] * (n - 5), np.int32)
    r = dict(t=torch.as_tensor(t).to(dev), rank=torch.as_tensor(rank).to(dev), t_host=t, rank_host=rank, rows=rows,
             cur_obs=z(n, D), actions=z(n, A), obs_next=z(n, D), rewards=z(n), dones=z(n), obs_reset=None, n_step=N,
             cursor=0, hist=z(n, Hd, C, Hh, W, dtype=torch.uint8), hist_pos=pos,
             obs_pixel=z(n, S * C, Hh, W, dtype=torch.uint8), frames_next=torch.full((n, C, Hh, W), 9, dtype=torch.uint8,
                                                                                      device=dev), frames_reset=None)
    F = C * Hh * W
    if ppo:
        r.update(pds=z(n, 2 * A), advance=3,
                 carry={'obs': z(n, N, D), 'actions': z(n, N, A), 'rewards': z(n, N), 'pds': z(n, N, 2 * A)},
                 tables={'obs': z(cap, N * D), 'obs_next': z(cap, D), 'actions': z(cap, N * A), 'rewards': z(cap, N),
                         'dones': z(cap, N), 'pds': z(cap, N * 2 * A), 'pixel': z(cap, N * S * F, dtype=torch.uint8),
                         'pixel_next': z(cap, S * F, dtype=torch.uint8)})
    else:
        r.update(gpow=torch.ones(N, dtype=torch.float64, device=dev),
                 carry={'obs': z(n, N, D), 'actions': z(n, N, A), 'rewards': z(n, N)},
                 tables={'obs': z(cap, D), 'obs_next': z(cap, D), 'actions': z(cap, A), 'rewards': z(cap, 1),
                         'dones': z(cap, 1), 'pixel': z(cap, S * F, dtype=torch.uint8),
                         'pixel_next': z(cap, S * F, dtype=torch.uint8)})
    return r


@pytest.mark.parametrize('ppo', [True, False])
def test_bad_arguments_return_the_documented_codes_without_launching(ppo):
    from surreal_amd import _lib as L, kernels as KN
    K = KN.HipKernels()
    launch = K.record_ppo_pixel_window_step if ppo else K.record_ddpg_pixel_nstep_step
    for change in (dict(Hd=6),                                    # hist_len < n_step + S
                   dict(pos=7), dict(pos=-1),                     # hist_pos out of range
                   dict(n=9),                                     # n > capacity
                   dict(rows=3), dict(rows=1)):                   # closing actors != rows
        r = _launch_args(ppo, **change)
        with pytest.raises(L.SmxError, match=r'rc=-2 '):          # SMX_E_SHAPE
            launch(r)
        torch.cuda.synchronize()
        for k, x in list(r['tables'].items()) + [('hist', r['hist']), ('obs_pixel', r['obs_pixel'])]:
            assert not x.any(), (change, k)                       # nothing was launched
    r = _launch_args(ppo)
    launch(r)                                                     # the same block, unchanged, is taken
    torch.cuda.synchronize()
    assert bool((r['hist'][:, 1] == 9).all()) and bool((r['obs_pixel'][:, -1] == 9).all())
    assert r['tables']['pixel_next'][:2, -16:].eq(9).all() and not r['tables']['pixel_next'][2:].any()
