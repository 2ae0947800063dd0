"""
The device recorders with a camera (surreal_amd/env/device_recorder.py with ``pixel=(C, H, W), frame_stacks=S``:
smx_record_ppo_pixel_window_step / smx_record_ddpg_pixel_nstep_step) against the host chains they replace, shared by the
CPU tier (test_pixel_recorder_cpu.py) and the GPU tier (test_gpu_pixel_recorder.py):

  * ``ScriptedCameraEnv`` -- recorder_cases.ScriptedEnv plus a seeded uint8 frame per observation (ONE raw frame:
    ``obs['pixel']['camera0']`` [C, H, W]); episode lengths cycle per actor, so the clocks of n of them diverge;
  * ``PixelRecorderCpuKernels`` -- the torch-CPU double of the two new entry points (a subclass of RecorderCpuKernels):
    the slot and stacking rules of the header, actor by actor;
  * ``host_ppo_pixel`` / ``host_ddpg_pixel`` -- n ScriptedCameraEnv behind EpisodeMonitor, FrameStackWrapper (concatenate
    on env) and ExpSenderWrapperMultiStepMovingWindowWithInfo / ExpSenderWrapperSSARNStepBootstrap, stepped in actor order
    into ONE list sink -> the experiences in insertion order, the RAW step stream the recorder is fed (the last C channels
    of a stacked observation are its newest raw frame) and the chain's stacked observation after every step;
  * ``device_ppo_pixel`` / ``device_ddpg_pixel`` -- that stream through a recorder into a replay's ring, the acting
    observation checked after every step.
"""
import collections
import types

import numpy as np
import torch

import helpers as H
import ppo_window_cases as PW
import recorder_cases as RC
from surreal_amd.env import stack_sources

LENGTHS = [2, 4, 9, 5, 14]             # for N = 4, S <= 3: shorter than S, shorter than N, equal to N, closing on the
#                                        terminal step, long
DDPG_LENGTHS = [2, 3, 9, 5, 14]


class ScriptedCameraEnv(RC.ScriptedEnv):
    """ScriptedEnv whose observation also carries ONE raw frame, uint8 draws of the same RandomState"""

    def __init__(self, seed, lengths, D=7, pixel=(1, 4, 4), rotation=None, log=None, tag=None):
        super().__init__(seed, lengths, D, rotation, log, tag)
        self.pixel = tuple(pixel)

    def _observe(self):
        obs = super()._observe()
        obs['pixel'] = collections.OrderedDict(camera0=self.rs.randint(0, 256, self.pixel).astype(np.uint8))
        return obs


def raw_frame(obs, C):
    """the newest raw frame of a stacked observation: its last C channels"""
    return np.asarray(obs['pixel']['camera0'])[-C:]


# ---- the torch-CPU double ----------------------------------------------------------------------------------------------
class PixelRecorderCpuKernels(RC.RecorderCpuKernels):
    name = 'torch-cpu-double+pixel-recorder'

    def __init__(self):
        super().__init__()
        self.pixel_launches = 0

    def _frames(self, r, N, frames_per_row, closing_tops):
        """the frame half of both entry points.  closing_tops(tau) -> the episode steps whose stacked observations make
        up the closing experience's `pixel` (None: the clock closes nothing at tau)"""
        hist, obs_pix, tabs = r['hist'], r['obs_pixel'], r['tables']
        n, Hd, C, Hh, W = hist.shape
        S = obs_pix.shape[1] // C
        pos = int(r['hist_pos'])
        cap = tabs['obs'].shape[0]
        assert Hd >= N + S and 0 <= pos < Hd and n <= cap
        assert hist.dtype == obs_pix.dtype == tabs['pixel'].dtype == tabs['pixel_next'].dtype == torch.uint8
        assert tuple(tabs['pixel'].shape) == (cap, frames_per_row * S * C * Hh * W)
        assert tuple(tabs['pixel_next'].shape) == (cap, S * C * Hh * W)
        nxt_in = r['frames_next'].reshape(n, C, Hh, W)
        reset_in = None if r.get('frames_reset') is None else r['frames_reset'].reshape(n, C, Hh, W)
        assert nxt_in.dtype == torch.uint8
        for a in range(n):
            clock = self._clock(r, a)
            if clock is None:
                continue
            tau, rank = clock
            restart = bool(r['dones'][a] != 0) and reset_in is not None

            def frame(u):
                # step tau + 1's frame is the input; older ones sit in slot (p - tau + u) mod Hd
                return nxt_in[a] if u == tau + 1 else hist[a, (pos - tau + u) % Hd]

            def stacked(top):
                return torch.cat([frame(u) for u in stack_sources(top, S)], dim=0)
            nxt = stacked(tau + 1)
            tops = closing_tops(tau)
            if rank >= 0 and tops is not None:
                row = (int(r['cursor']) + rank) % cap
                tabs['pixel'][row] = torch.stack([stacked(u) for u in tops]).reshape(-1)
                tabs['pixel_next'][row] = nxt.reshape(-1)
            # the terminal frame never enters the history
            hist[a, (pos + 1) % Hd] = reset_in[a] if restart else nxt_in[a]
            obs_pix[a] = reset_in[a].repeat(S, 1, 1) if restart else nxt

    def record_ppo_pixel_window_step(self, r, copy_workgroups=0, monitor=None):
        self.pixel_launches += 1
        N, adv = int(r['n_step']), int(r['advance'])

        def tops(tau):
            j = tau + 1 - N
            return [j + u for u in range(N)] if j >= 0 and j % adv == 0 else None
        self._frames(r, N, N, tops)
        self.record_ppo_window_step(r, copy_workgroups=copy_workgroups, monitor=monitor)

    def record_ddpg_pixel_nstep_step(self, r, copy_workgroups=0, monitor=None):
        self.pixel_launches += 1
        N = int(r['n_step'])
        assert 0 <= copy_workgroups <= 1024
        self._frames(r, N, 1, lambda tau: [tau - N + 1] if tau >= N - 1 else None)
        self.record_ddpg_nstep_step(r, monitor=monitor)


# ---- the host side: n chains, one sink ---------------------------------------------------------------------------------
def _drive(n, D, pixel, S, lengths, steps, seed, wrap, act):
    """recorder_cases._drive for n ScriptedCameraEnv behind EpisodeMonitor, FrameStackWrapper and `wrap`"""
    from surreal_amd.env import EpisodeMonitor, FrameStackWrapper
    from surreal_amd.session import Config
    C = pixel[0]
    exps, monitors, ws = [], [], []
    for a in range(n):
        mon = EpisodeMonitor(ScriptedCameraEnv(seed + a, lengths, D, pixel, rotation=a))
        monitors.append(mon)
        stack = FrameStackWrapper(mon, Config(frame_stacks=S, frame_stack_concatenate_on_env=True))
        ws.append(wrap(stack, exps.append))
    first = [w.reset()[0] for w in ws]
    u8 = lambda *s: np.zeros(s, np.uint8)  # noqa: E731
    s = types.SimpleNamespace(
        n=n, D=D, pixel=tuple(pixel), S=S, steps=steps, exps=exps, monitors=monitors,
        first=np.stack([RC.flat(o) for o in first]), first_frames=np.stack([raw_frame(o, C) for o in first]),
        obs_next=np.zeros((steps, n, D), np.float32), obs_reset=np.zeros((steps, n, D), np.float32),
        rewards=np.zeros((steps, n), np.float32), dones=np.zeros((steps, n), bool),
        frames_next=u8(steps, n, *pixel), frames_reset=u8(steps, n, *pixel),
        acting=u8(steps, n, S * C, *pixel[1:]), count=[])
    for o in first:                                   # a reset fills the stack with the first frame
        assert np.array_equal(np.asarray(o['pixel']['camera0']), np.tile(raw_frame(o, C), (S, 1, 1)))
    for step in range(steps):
        for a, w in enumerate(ws):
            obs, reward, done, _ = w.step(act(step, a))
            s.obs_next[step, a], s.rewards[step, a], s.dones[step, a] = RC.flat(obs), reward, done
            s.frames_next[step, a] = raw_frame(obs, C)
            if done:
                obs = w.reset()[0]
                s.obs_reset[step, a], s.frames_reset[step, a] = RC.flat(obs), raw_frame(obs, C)
            s.acting[step, a] = np.asarray(obs['pixel']['camera0'])   # what the chain's agent acts on next
        s.count.append(len(exps))
    return s


def cam(obs):
    return np.asarray(obs['pixel']['camera0'])


def host_ppo_pixel(n, D, A, pixel, S, lengths, steps, n_step, stride, rnn_hidden=0, seed=0):
    """recorder_cases.host_ppo with the camera: `fields` also holds pixel uint8 [windows, n_step, S*C, H, W] and
    pixel_next [windows, 1, S*C, H, W]"""
    from surreal_amd.env import ExpSenderWrapperMultiStepMovingWindowWithInfo
    lc, ec, sc = PW.configs(D, A, n_step, stride, rnn_hidden=rnn_hidden or None)
    rs = np.random.RandomState(1000 + seed)
    actions = rs.uniform(-1, 1, (steps, n, A)).astype(np.float32)
    pds = rs.standard_normal((steps, n, 2 * A)).astype(np.float32)
    h = rs.standard_normal((steps, n, rnn_hidden)).astype(np.float32)
    c = rs.standard_normal((steps, n, rnn_hidden)).astype(np.float32)

    def act(s, a):
        once = [h[s, a][None].copy(), c[s, a][None].copy()] if rnn_hidden else []
        return actions[s, a].copy(), [once, [pds[s, a].copy()]]
    st = _drive(n, D, pixel, S, lengths, steps, seed,
                lambda env, sink: ExpSenderWrapperMultiStepMovingWindowWithInfo(env, lc, sc, sink=sink), act)
    st.A, st.actions, st.pds, st.h, st.c, st.rnn_hidden = A, actions, pds, h, c, rnn_hidden
    x = st.exps
    f = {'obs': [[RC.flat(o) for o in e['obs']] for e in x], 'obs_next': [[RC.flat(e['obs_next'])] for e in x],
         'actions': [e['actions'] for e in x], 'rewards': [e['rewards'] for e in x], 'dones': [e['dones'] for e in x],
         'pds': [[p[0] for p in e['persistent_infos']] for e in x]}
    if rnn_hidden:
        f['cells'] = [e['onetime_infos'] for e in x]                  # [2, 1, Hl]
    shapes = {'obs': (n_step, D), 'obs_next': (1, D), 'actions': (n_step, A), 'rewards': (n_step,), 'dones': (n_step,),
              'pds': (n_step, 2 * A), 'cells': (2, 1, rnn_hidden)}
    st.fields = {k: np.asarray(v, dtype=np.float32).reshape((len(x),) + shapes[k]) for k, v in f.items()}
    stacked = (S * pixel[0],) + tuple(pixel[1:])
    st.fields['pixel'] = np.asarray([[cam(o) for o in e['obs']] for e in x], np.uint8).reshape(
        (len(x), n_step) + stacked)
    st.fields['pixel_next'] = np.asarray([cam(e['obs_next']) for e in x], np.uint8).reshape((len(x), 1) + stacked)
    return st


def host_ddpg_pixel(n, D, A, pixel, S, lengths, steps, n_step, gamma, seed=0):
    """recorder_cases.host_ddpg with the camera: pixel / pixel_next uint8 [rows, S*C, H, W]"""
    import ddpg_rollout_cases as DC
    from surreal_amd.env import ExpSenderWrapperSSARNStepBootstrap
    lc, ec, sc = DC.configs(D, A, n, n_step=n_step, gamma=gamma, folder='surreal_amd_recorder')
    actions = np.random.RandomState(2000 + seed).uniform(-1, 1, (steps, n, A)).astype(np.float32)
    st = _drive(n, D, pixel, S, lengths, steps, seed,
                lambda env, sink: ExpSenderWrapperSSARNStepBootstrap(env, lc, sc, sink=sink),
                lambda s, a: actions[s, a].copy())
    st.A, st.actions = A, actions
    x = st.exps
    stacked = (S * pixel[0],) + tuple(pixel[1:])
    st.fields = {'obs': np.asarray([RC.flat(e['obs'][0]) for e in x], np.float32).reshape(len(x), D),
                 'obs_next': np.asarray([RC.flat(e['obs'][1]) for e in x], np.float32).reshape(len(x), D),
                 'actions': np.asarray([e['action'] for e in x], np.float32).reshape(len(x), A),
                 'rewards': np.asarray([np.float32(e['reward']) for e in x], np.float32),
                 'dones': np.asarray([float(e['done']) for e in x], np.float32),
                 'pixel': np.asarray([cam(e['obs'][0]) for e in x], np.uint8).reshape((len(x),) + stacked),
                 'pixel_next': np.asarray([cam(e['obs'][1]) for e in x], np.uint8).reshape((len(x),) + stacked)}
    return st


# ---- the device side ---------------------------------------------------------------------------------------------------
def _check_acting(rec, st, s):
    """after step s: the recorder's observation is the chain's next stacked observation (and low-dimensional one)"""
    obs = rec.observation
    assert list(obs) == ['pixel', 'low_dim'] and list(obs['pixel']) == ['camera0']
    assert torch.equal(obs['pixel']['camera0'].cpu(), torch.as_tensor(st.acting[s])), s
    low = np.where(st.dones[s][:, None], st.obs_reset[s], st.obs_next[s])
    assert torch.equal(obs['low_dim']['flat_inputs'].cpu(), torch.as_tensor(low)), s


def device_ppo_pixel(st, replay, n_step, stride, monitor=None, resume_at=(), copy_workgroups=0, as_tensors=False,
                     hist_len=None):
    """the stream of host_ppo_pixel through a DeviceWindowRecorder with a camera into `replay` -> (recorder, rows);
    arguments as recorder_cases.device_ppo.  frames_reset is passed on every step (HostVecEnv does): the recorder sends
    it on only where some actor is done"""
    from surreal_amd.env import DeviceWindowRecorder
    make = lambda: DeviceWindowRecorder(st.n, st.D, st.A, n_step, stride, rnn_hidden=st.rnn_hidden,  # noqa: E731
                                        pixel=st.pixel, frame_stacks=st.S)
    rec = make()
    assert rec.hist_len == n_step + st.S == (hist_len or rec.hist_len)    # the minimum the kernels take
    rec.begin(st.first, st.first_frames)
    total = 0
    put = RC._dev if as_tensors else (lambda x: x)
    for s in range(st.steps):
        if s in resume_at:
            sd = rec.state_dict()
            rec = make()
            rec.load_state_dict(sd)
        cells = (RC._dev(st.h[s]), RC._dev(st.c[s])) if st.rnn_hidden else None
        total += rec.record(replay, RC._dev(st.actions[s]), RC._dev(st.pds[s]), put(st.rewards[s]), st.dones[s],
                            put(st.obs_next[s]), put(st.obs_reset[s]), cells_before=cells, monitor=monitor,
                            copy_workgroups=copy_workgroups, frames_next=put(st.frames_next[s]),
                            frames_reset=put(st.frames_reset[s]))
        _check_acting(rec, st, s)
    return rec, total


def device_ddpg_pixel(st, replay, n_step, gamma, monitor=None, resume_at=(), copy_workgroups=0):
    from surreal_amd.env import DeviceNStepRecorder
    make = lambda: DeviceNStepRecorder(st.n, st.D, st.A, n_step, gamma, pixel=st.pixel,  # noqa: E731
                                       frame_stacks=st.S)
    rec = make()
    rec.begin(st.first, st.first_frames)
    total = 0
    for s in range(st.steps):
        if s in resume_at:
            sd = rec.state_dict()
            rec = make()
            rec.load_state_dict(sd)
        done = st.dones[s].any()
        total += rec.record(replay, RC._dev(st.actions[s]), st.rewards[s], st.dones[s], st.obs_next[s],
                            st.obs_reset[s] if done else None, monitor=monitor, frames_next=st.frames_next[s],
                            frames_reset=st.frames_reset[s] if done else None, copy_workgroups=copy_workgroups)
        _check_acting(rec, st, s)
    return rec, total


def fifo(D, A, n_step, stride, memory_size, rnn_hidden=0):
    return RC.fifo(D, A, n_step, stride, memory_size, rnn_hidden)


def assert_ring_equals(replay, fields, capacity, cursor0=0):
    """recorder_cases.assert_ring_equals keeping each field's dtype (the uint8 frames): torch.equal per field"""
    got = H.device_ring(replay)
    assert set(got) == set(fields), (sorted(got), sorted(fields))
    for k, v in fields.items():
        rows = v.reshape(v.shape[0], int(np.prod(v.shape[1:])))
        want = np.zeros((capacity, rows.shape[1]), v.dtype)
        for i in range(rows.shape[0]):
            want[(cursor0 + i) % capacity] = rows[i]
        g, w = torch.as_tensor(got[k]), torch.as_tensor(want)
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), (k, np.argwhere(got[k] != want)[:5].tolist())
