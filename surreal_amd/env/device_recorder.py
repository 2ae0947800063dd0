"""
Recording the steps of n HOST-stepped environments (GymAdapter, DMControlAdapter, RobosuiteWrapper: simulators that end
their episodes whenever they like) into the replays' device rings: what n experience wrappers do per step on the host
(exp_sender_wrapper.py: a ring of n_step slots per actor, one ``insert`` per experience) as ONE launch per step for all
actors (csrc/smx_record.hip), every actor on an episode clock of its own.  The observation is one flat low-dimensional
array and, with ``pixel=(C, H, W)``, ONE raw uint8 camera frame per step: the same launch then keeps a frame history per
actor, stacks the acting observation (FrameStackWrapper's rule, ``frame_stacks`` frames on the channel axis) and writes
the closing experiences' stacked ``pixel`` / ``pixel_next`` into the ring.

The host keeps the clocks -- it sees the dones -- and per step computes who closes an experience and where it goes:

  PPO   actor a at step t of its episode closes window t + 1 - N iff that is >= 0 and a multiple of advance
  DDPG  actor a emits transition t - N + 1 iff t >= N - 1
  rank  the actor's position among this step's closing actors in ascending actor order (-1: none); its row is
        (cursor + rank) % capacity, so a step's rows are dense and in the order n host wrappers stepped in actor order
        would have inserted them.

What the device needs of a step travels in ONE pinned staging set -- clocks, ranks, dones and whichever of rewards /
obs_next / obs_reset (and, last, the camera's frames_next / frames_reset) are host arrays -- by one copy.  There are
two sets, each with an event recorded behind its copy that is waited on before the host writes the set again; nothing
else synchronises.
"""
import collections

import numpy as np
import torch

from surreal_amd import kernels as KN
from .exp_sender_wrapper import window_advance


def closing_ranks(closes):
    """closes bool [n] -> (rank int32 [n]: position among the closing actors in actor order, -1 elsewhere; their number)"""
    closes = np.asarray(closes, dtype=bool)
    rank = np.where(closes, np.cumsum(closes) - 1, -1).astype(np.int32)
    return rank, int(closes.sum())


def _pad4(words):
    return -(-words // 4) * 4                 # every field starts on 16 bytes


class _StagingSet(object):
    """one pinned host buffer and its device twin: t | rank (int32 [n]) | dones | rewards (fp32 [n]) | obs_next |
    obs_reset (fp32 [n, D]) and, with a camera of F bytes a frame, | frames_next | frames_reset (uint8 [n, F]); the host
    side as numpy views, the device side as tensors"""
    FIELDS = ('t', 'rank', 'dones', 'rewards', 'obs_next', 'obs_reset')
    CAMERA = ('frames_next', 'frames_reset')

    def __init__(self, n, D, device, F=0):
        cuda = device.type == 'cuda'
        self.fields = self.FIELDS + (self.CAMERA if F else ())
        sizes = (n, n, n, n, n * D, n * D) + ((-(-n * F // 4),) * 2 if F else ())
        self.host = torch.zeros(sum(_pad4(s) for s in sizes), dtype=torch.int32, pin_memory=cuda)
        self.dev = torch.zeros(self.host.numel(), dtype=torch.int32, device=device)
        self.event = torch.cuda.Event() if cuda else None
        self.in_flight = False
        words = self.host.numpy()
        self.h, self.d, self.end = {}, {}, {}
        off = 0
        for name, size in zip(self.fields, sizes):
            h, d = words[off:off + size], self.dev[off:off + size]
            if name in self.CAMERA:
                h, d = h.view(np.uint8)[:n * F].reshape(n, F), d.view(torch.uint8)[:n * F].view(n, F)
            elif name not in ('t', 'rank'):
                h, d = h.view(np.float32), d.view(torch.float32)
            if name in ('obs_next', 'obs_reset'):
                h, d = h.reshape(n, D), d.view(n, D)
            self.h[name], self.d[name] = h, d
            off += _pad4(size)
            self.end[name] = off

    def wait(self):
        """until the copy that last read this set's host side is done"""
        if self.in_flight and self.event is not None:
            self.event.synchronize()
        self.in_flight = False

    def upload(self, last):
        """the one copy of a step: everything up to field `last`"""
        words = self.end[last]
        self.dev[:words].copy_(self.host[:words], non_blocking=True)
        if self.event is not None:
            self.event.record()
        self.in_flight = True


class _DeviceRecorder(object):
    """what the two recorders share: the clocks, cur_obs, the staging sets and, with a camera, the frame history"""

    def __init__(self, n, D, A, n_step, kernels=None, device=None, pixel=None, frame_stacks=1):
        self.n, self.D, self.A, self.n_step = int(n), int(D), int(A), int(n_step)
        if min(self.n, self.D, self.A, self.n_step) < 1:
            raise ValueError('recorder: n, D, A and n_step must be positive, got %r' % ((n, D, A, n_step),))
        self.K = kernels if kernels is not None else KN.default_kernels()
        self.device = torch.device(device if device is not None else KN.default_device())
        self.cur_obs = torch.zeros(self.n, self.D, device=self.device)
        self.t = np.zeros(self.n, dtype=np.int32)            # each actor's step within its episode
        self.carry = {}
        self.pixel = None if pixel is None else tuple(int(v) for v in pixel)
        self.frame_stacks = int(frame_stacks) if pixel is not None else 1
        self.F = 0
        if self.pixel is not None:
            if len(self.pixel) != 3 or min(self.pixel) < 1 or self.frame_stacks < 1:
                raise ValueError('recorder: pixel must be (C, H, W) and frame_stacks positive, got %r, %r'
                                 % (pixel, frame_stacks))
            C, H, W = self.pixel
            self.F = C * H * W
            # the raw frames of the last n_step + S steps, actor a's current one in slot hist_pos (one counter: every
            # actor receives one frame per step); the stacked observation the actors act on next
            self.hist_len = self.n_step + self.frame_stacks
            self.hist = torch.zeros(self.n, self.hist_len, C, H, W, dtype=torch.uint8, device=self.device)
            self.obs_pixel = torch.zeros(self.n, self.frame_stacks * C, H, W, dtype=torch.uint8, device=self.device)
            self.hist_pos = 0
        self._sets = [_StagingSet(self.n, self.D, self.device, self.F) for _ in range(2)]
        self._next = 0
        # a frame-pool replay (replay.device_frame_pool): the actors whose current frame (hist's slot hist_pos: begin,
        # reset) has yet to enter the pool, and those whose episode restarted on the frame they have
        self._pool = None
        self._prime = np.zeros(self.n, dtype=bool)
        self._refirst = np.zeros(self.n, dtype=bool)

    @property
    def observation(self):
        """what every actor acts on next (act_batch reads it; record() moves it on): [n, D] on the device, with a camera
        the nested {'pixel': {'camera0': uint8 [n, S*C, H, W]}, 'low_dim': {'flat_inputs': [n, D]}}"""
        if self.pixel is None:
            return self.cur_obs
        return collections.OrderedDict(pixel=collections.OrderedDict(camera0=self.obs_pixel),
                                       low_dim=collections.OrderedDict(flat_inputs=self.cur_obs))

    def _on_device(self, x):
        return torch.is_tensor(x) and x.device.type == self.device.type

    def _device_rows(self, x, width):
        """a host array or a tensor -> fp32 [n, width] on the device (begin / reset: not the per-step path)"""
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        x = x.to(device=self.device, dtype=torch.float32)
        if x.numel() != self.n * width:
            raise ValueError('recorder: expected %d x %d values, got %s' % (self.n, width, tuple(x.shape)))
        return x.reshape(self.n, width)

    def _device_frames(self, frames):
        """host or device uint8 frames -> uint8 [n, C, H, W] on the device (begin / reset: not the per-step path)"""
        if frames is None:
            raise ValueError('recorder: a recorder with a camera needs the frames')
        if not torch.is_tensor(frames):
            frames = np.asarray(frames)
            if frames.dtype != np.uint8:
                raise ValueError('recorder: frames must be uint8, got %s' % frames.dtype)
            frames = torch.as_tensor(np.ascontiguousarray(frames))
        if frames.dtype != torch.uint8 or frames.numel() != self.n * self.F:
            raise ValueError('recorder: expected uint8 frames %s, got %s %s'
                             % ((self.n,) + self.pixel, frames.dtype, tuple(frames.shape)))
        return frames.to(self.device).reshape((self.n,) + self.pixel)

    def _no_frames(self, frames):
        if frames is not None:
            raise ValueError('recorder: frames given to a recorder without a camera')

    def begin(self, obs, frames=None):
        """the first observations [n, D] of n fresh episodes (with a camera: their first frames uint8 [n, C, H, W], into
        the history and frame_stacks times into the acting observation); all clocks to 0"""
        if self.pixel is None:
            self._no_frames(frames)
        else:
            f = self._device_frames(frames)
            self.hist_pos = 0
            self.hist[:, 0].copy_(f)
            self.obs_pixel.copy_(f.repeat(1, self.frame_stacks, 1, 1))
            self._prime[:] = True
        self.cur_obs.copy_(self._device_rows(obs, self.D))
        self.t[:] = 0

    def reset(self, mask=None, obs=None, frames=None):
        """restart the episodes of the actors in `mask` (host bool [n]; None: all) outside record() -- their clocks go to
        0 and their open windows / transitions are dropped; obs [n, D]: their first observations (the masked rows); with
        a camera frames [n, C, H, W] goes with obs: their first frames"""
        mask = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(self.n)
        if self.pixel is None:
            self._no_frames(frames)
        elif (obs is None) != (frames is None):
            raise ValueError('recorder: with a camera, obs and frames restart an episode together')
        rows = self._device_rows(obs, self.D) if obs is not None else None
        f = self._device_frames(frames) if frames is not None else None
        self.t[mask] = 0
        if self.pixel is not None:
            if f is not None:
                self._prime |= mask
            else:
                self._refirst |= mask
        if obs is not None:
            m = torch.as_tensor(mask).to(self.device)
            self.cur_obs.copy_(torch.where(m.view(-1, 1), rows, self.cur_obs))
            if f is not None:
                m4 = m.view(-1, 1, 1, 1)
                slot = self.hist[:, self.hist_pos]
                slot.copy_(torch.where(m4, f, slot))
                self.obs_pixel.copy_(torch.where(m4, f.repeat(1, self.frame_stacks, 1, 1), self.obs_pixel))

    def state_dict(self):
        sd = {'t': self.t.copy(), 'cur_obs': self.cur_obs.detach().cpu().clone(),
              'carry': {k: v.detach().cpu().clone() for k, v in self.carry.items()}}
        if self.pixel is not None:
            sd.update(hist=self.hist.cpu().clone(), hist_pos=int(self.hist_pos), obs_pixel=self.obs_pixel.cpu().clone())
        return sd

    def load_state_dict(self, sd):
        if set(sd['carry']) != set(self.carry):
            raise ValueError('recorder: the state holds rings %s, this recorder %s'
                             % (sorted(sd['carry']), sorted(self.carry)))
        if ('hist' in sd) != (self.pixel is not None):
            raise ValueError('recorder: the state %s a camera, this recorder %s one'
                             % (('has', 'has not') if 'hist' in sd else ('has not', 'has')))
        if self.pixel is not None:
            hist, obs_pixel = torch.as_tensor(sd['hist']), torch.as_tensor(sd['obs_pixel'])
            if tuple(hist.shape) != tuple(self.hist.shape) or tuple(obs_pixel.shape) != tuple(self.obs_pixel.shape):
                raise ValueError('recorder: the state holds frames %s / %s, this recorder %s / %s'
                                 % (tuple(hist.shape), tuple(obs_pixel.shape), tuple(self.hist.shape),
                                    tuple(self.obs_pixel.shape)))
            if not 0 <= int(sd['hist_pos']) < self.hist_len:
                raise ValueError('recorder: hist_pos %r outside the history of %d' % (sd['hist_pos'], self.hist_len))
            self.hist.copy_(hist)
            self.obs_pixel.copy_(obs_pixel)
            self.hist_pos = int(sd['hist_pos'])
        self.t[:] = np.asarray(sd['t'], dtype=np.int32).reshape(self.n)
        self.cur_obs.copy_(self._device_rows(sd['cur_obs'], self.D))
        for k, v in self.carry.items():
            v.copy_(torch.as_tensor(sd['carry'][k]).reshape(v.shape))

    # ---- one step -------------------------------------------------------------------------------------------------
    def _closes(self, t):
        raise NotImplementedError

    def _stage(self, rewards, dones, obs_next, obs_reset, frames_next=None, frames_reset=None):
        """this step's clocks, ranks, dones and host arrays into the next staging set and on their way ->
        (dones bool [n], rows, {name: device tensor} for the launch, the set's host t / rank).  With a camera the frames
        travel last; frames_reset only on a step where some actor is done"""
        n, D, F = self.n, self.D, self.F
        dones = np.asarray(dones).astype(bool).reshape(n)
        if obs_reset is None and dones.any():
            raise ValueError('record: actors %s are done and there is no obs_reset to go on from'
                             % np.flatnonzero(dones).tolist())
        if self.pixel is None:
            if frames_next is not None or frames_reset is not None:
                raise ValueError('record: frames given to a recorder without a camera')
        else:
            if frames_next is None:
                raise ValueError('record: frames_next is required with a camera')
            if frames_reset is None and dones.any():
                raise ValueError('record: actors %s are done and there is no frames_reset to go on from'
                                 % np.flatnonzero(dones).tolist())
            if not dones.any():
                frames_reset = None
            for name, x in (('frames_next', frames_next), ('frames_reset', frames_reset)):
                if x is not None and (x.dtype != (torch.uint8 if torch.is_tensor(x) else np.uint8) or
                                      (x.numel() if torch.is_tensor(x) else x.size) != n * F):
                    raise ValueError('record: %s must be uint8 %s, got %s %s'
                                     % (name, (n,) + self.pixel, x.dtype, tuple(x.shape)))
        rank, rows = closing_ranks(self._closes(self.t))
        s = self._sets[self._next]
        self._next ^= 1
        s.wait()
        s.h['t'][:] = self.t
        s.h['rank'][:] = rank
        s.h['dones'][:] = dones
        dev, last = {'t': s.d['t'], 'rank': s.d['rank'], 'dones': s.d['dones']}, 'dones'
        for name, x, width in (('rewards', rewards, 1), ('obs_next', obs_next, D), ('obs_reset', obs_reset, D)):
            if x is None:
                if name != 'obs_reset':
                    raise ValueError('record: %s is required' % name)
                dev[name] = None
            elif self._on_device(x):
                if x.numel() != n * width:
                    raise ValueError('record: %s has %d values, expected %d' % (name, x.numel(), n * width))
                dev[name] = x.to(torch.float32).contiguous()
            else:
                x = x.numpy() if torch.is_tensor(x) else np.asarray(x)
                if x.size != n * width:
                    raise ValueError('record: %s has shape %s, expected %d values' % (name, x.shape, n * width))
                s.h[name][...] = x.reshape(s.h[name].shape)
                dev[name], last = s.d[name], name
        if self.pixel is not None:
            for name, x in (('frames_next', frames_next), ('frames_reset', frames_reset)):
                if x is None:
                    dev[name] = None
                elif self._on_device(x):
                    dev[name] = x.contiguous().view((n,) + self.pixel)
                else:
                    x = x.numpy() if torch.is_tensor(x) else np.asarray(x)
                    s.h[name][...] = x.reshape(n, F)
                    dev[name], last = s.d[name].view((n,) + self.pixel), name
        s.upload(last)
        return dones, rows, dev, s.h['t'], s.h['rank']

    def _step_rows(self, x, width, name):
        if not self._on_device(x) or x.numel() != self.n * width:
            raise ValueError('record: %s must be a device tensor of %d x %d values' % (name, self.n, width))
        return x.to(torch.float32).contiguous()

    def _camera_shapes(self, frames_per_row):
        """the ring's uint8 camera fields next to self.shapes: pixel (frames_per_row stacked frames; None: one, without
        the axis) and pixel_next"""
        C, H, W = self.pixel
        stacked = (self.frame_stacks * C, H, W)
        self.shapes['pixel'] = stacked if frames_per_row is None else (frames_per_row,) + stacked
        self.shapes['pixel_next'] = stacked if frames_per_row is None else (1,) + stacked
        self.dtypes = {'pixel': torch.uint8, 'pixel_next': torch.uint8}

    def _ring(self, replay, rows, shapes):
        if self.pixel is None:
            tables, cursor, cap = replay.reserve_ring(rows, shapes)
        else:
            tables, cursor, cap = replay.reserve_ring(rows, shapes, self.dtypes)
        if self.n > cap:
            raise ValueError('record: %d actors exceed the replay ring of %d rows (all of them may close in one step)'
                             % (self.n, cap))
        return tables, cursor

    def _camera(self, dev):
        """the camera entries of a launch's argument dict"""
        return dict(dev, hist=self.hist, hist_pos=self.hist_pos, obs_pixel=self.obs_pixel)

    def _moved(self, dones, monitor):
        """after the launch: the clocks, the history's counter, the monitor's step count"""
        if monitor is not None:
            monitor.count_steps(1)
        if self.pixel is not None:
            self.hist_pos = (self.hist_pos + 1) % self.hist_len
        self._advance(dones)

    def _advance(self, dones):
        self.t = np.where(dones, 0, self.t + 1).astype(np.int32)

    # ---- the frame-pool layout (replay/frame_pool.py) -------------------------------------------------------------
    def _pool_reserve(self, replay, dones, rank_host, rows, shapes):
        """one DDPG step into a frame-pool replay, before its launch: the actors' counters f (newest frame) and first
        (the episode's reset frame) on the host and -- two buffers [2, n], swapped per launch -- on the device; the
        step's plan for the replay's ledger (reserve_frame_pool retires what the step overwrites); the frames begin() /
        reset() left in hist's current slot enter the pool first -> reserve_frame_pool's handle with the launch's
        counters_in / counters_out"""
        from surreal_amd.replay.frame_pool import oldest_frame
        n, N, S = self.n, self.n_step, self.frame_stacks
        if n > replay.memory_size:
            raise ValueError('record: %d actors exceed the replay ring of %d rows (all of them may close in one step)'
                             % (n, replay.memory_size))
        pl = self._pool
        if pl is None or pl['replay'] is not replay:
            start = replay.frame_pool['counter'].copy() if replay.frame_pool is not None else np.full(n, -1, np.int64)
            pl = self._pool = dict(replay=replay, f=start, first=start.copy(), side=0,
                                   dev=[torch.zeros(2, n, dtype=torch.int64, device=self.device) for _ in range(2)])
            self._prime[:] = True
        f, first = pl['f'], pl['first']
        steps, prime = [], self._prime.copy()
        moved = prime.any() or self._refirst.any()
        if moved:
            f[prime] += 1
            first[prime | self._refirst] = f[prime | self._refirst]
            steps.append((0, f.copy(), f.copy()))
            self._prime[:] = False
            self._refirst[:] = False
        closes = np.asarray(rank_host) >= 0
        oldest = np.where(closes, oldest_frame(f + 1, first, N, S), np.iinfo(np.int64).max)
        after = f + np.where(dones, 2, 1)
        steps.append((rows, after, oldest))
        h = replay.reserve_frame_pool(steps, shapes, n, self.pixel, S, N)
        if moved:
            C, H, W = self.pixel
            idx = torch.as_tensor(np.flatnonzero(prime)).to(self.device)
            slots = torch.as_tensor(f[prime] % h['pool'].shape[1]).to(self.device)
            h['pool'].view(n, -1, C, H, W)[idx, slots] = self.hist[idx, self.hist_pos]
            pl['dev'][pl['side']].copy_(torch.as_tensor(np.stack([f, first])))
        h.update(counters_in=pl['dev'][pl['side']], counters_out=pl['dev'][pl['side'] ^ 1], frame_shape=self.pixel)
        pl['side'] ^= 1
        pl['first'] = np.where(dones, f + 2, first)
        pl['f'] = after
        return h


class DeviceWindowRecorder(_DeviceRecorder):
    """PPO's moving windows (ExpSenderWrapperMultiStepMovingWindowWithInfo) of n host-stepped actors, written into the
    FIFO replay's device ring in the layout SyntheticVecEnv.ppo_rollout_into uses: obs [N, D], obs_next [1, D], actions
    [N, A], rewards / dones [N], pds [N, 2A] and, with rnn_hidden, cells [2, 1, rnn_hidden] (one LSTM layer): the state
    before the window's first step.

        rec = DeviceWindowRecorder(n, D, A, n_step, stride)
        rec.begin(first_obs)
        actions, pds = agent.act_batch(rec.observation)
        ... step the environments with actions ...
        rec.record(replay, actions, pds, rewards, dones, obs_next, obs_reset)

    With pixel=(C, H, W), frame_stacks=S the actors have a camera: begin(first_obs, first_frames), `observation` the
    nested dict act_batch takes, record(..., frames_next=, frames_reset=) with ONE raw uint8 frame per actor and step,
    and the ring gains uint8 pixel [N, S*C, H, W] / pixel_next [1, S*C, H, W]: what FrameStackWrapper (concatenate on
    env) in front of the experience wrapper would have put there.
    """

    def __init__(self, n, D, A, n_step, stride, rnn_hidden=0, kernels=None, device=None, pixel=None, frame_stacks=1):
        super().__init__(n, D, A, n_step, kernels, device, pixel, frame_stacks)
        if int(stride) < 1:
            raise ValueError('stride %r for experience generation cannot be less than 1' % (stride,))
        self.stride, self.advance = int(stride), window_advance(n_step, stride)
        self.rnn_hidden = int(rnn_hidden or 0)
        n, N, D, A = self.n, self.n_step, self.D, self.A
        f = lambda *s: torch.zeros(*s, device=self.device)  # noqa: E731
        self.carry = {'obs': f(n, N, D), 'actions': f(n, N, A), 'rewards': f(n, N), 'pds': f(n, N, 2 * A)}
        self.shapes = {'obs': (N, D), 'obs_next': (1, D), 'actions': (N, A), 'rewards': (N,), 'dones': (N,),
                       'pds': (N, 2 * A)}
        if self.rnn_hidden:
            self.carry['cells'] = f(n, -(-N // self.advance), 2, self.rnn_hidden)
            self.shapes['cells'] = (2, 1, self.rnn_hidden)
        if self.pixel is not None:
            self._camera_shapes(N)

    def _closes(self, t):
        start = t + 1 - self.n_step
        return (start >= 0) & (start % self.advance == 0)

    def record(self, replay, actions, pds, rewards, dones, obs_next, obs_reset=None, cells_before=None, monitor=None,
               copy_workgroups=0, frames_next=None, frames_reset=None):
        """one step of all actors -> the number of windows written.  actions [n, A] / pds [n, 2A]: device tensors (what
        act_batch returned for `observation`); dones: host bool [n]; rewards [n], obs_next [n, D] (the terminal
        observation where done), obs_reset [n, D] (the first observation of the next episode: only the rows of done
        actors are read; required when any actor is done): host arrays or device tensors; cells_before: (h, c), each
        [n, rnn_hidden] (or [1, n, rnn_hidden]) on the device -- the LSTM state the step started from
        (PPOAgent.batch_cells_before); monitor: a DeviceEpisodeMonitor over the n actors.  With a camera: frames_next
        uint8 [n, C, H, W] (the frame after the step, the terminal one where done) and frames_reset (the next episode's
        first frame: only the rows of done actors are read; required when any actor is done), host arrays or device
        tensors; copy_workgroups then counts the workgroups per actor that move frames.  Steps that close nothing still
        launch: the rings, the history and `observation` move."""
        n, Hl = self.n, self.rnn_hidden
        if (cells_before is None) != (Hl == 0):
            raise ValueError('record: cells_before goes with rnn_hidden (%d)' % Hl)
        actions, pds = self._step_rows(actions, self.A, 'actions'), self._step_rows(pds, 2 * self.A, 'pds')
        hb = cb = None
        if Hl:
            hb, cb = (self._step_rows(x, Hl, 'cells_before') for x in cells_before)
        dones, rows, dev, t_host, rank_host = self._stage(rewards, dones, obs_next, obs_reset, frames_next, frames_reset)
        tables, cursor = self._ring(replay, rows, self.shapes)
        r = dict(dev, t_host=t_host, rank_host=rank_host, rows=rows, cur_obs=self.cur_obs, actions=actions, pds=pds,
                 h_before=hb, c_before=cb, n_step=self.n_step, advance=self.advance, carry=self.carry, tables=tables,
                 cursor=cursor)
        if self.pixel is None:
            self.K.record_ppo_window_step(r, copy_workgroups=copy_workgroups, monitor=monitor)
        else:
            self.K.record_ppo_pixel_window_step(self._camera(r), copy_workgroups=copy_workgroups, monitor=monitor)
        replay.commit_ring(rows)
        self._moved(dones, monitor)
        return rows


class DeviceNStepRecorder(_DeviceRecorder):
    """DDPG's n-step transitions (ExpSenderWrapperSSARNStepBootstrap, its fill-up discount exponents included) of n
    host-stepped actors, written into the uniform replay's device ring in SyntheticVecEnv.ddpg_rollout_into's layout: obs /
    obs_next [D], actions [A], rewards, dones.  The reward is the wrapper's fp64 sum in step order, rounded once.  With
    pixel=(C, H, W), frame_stacks=S (see DeviceWindowRecorder) also uint8 pixel / pixel_next [S*C, H, W] -- or, into a
    frame-pool replay (replay.device_frame_pool), every frame once in the replay's pool and two counters a row
    (smx_record_ddpg_pixel_pool_nstep_step): begin / record / observation / reset are the same calls."""

    def __init__(self, n, D, A, n_step, gamma, kernels=None, device=None, pixel=None, frame_stacks=1):
        super().__init__(n, D, A, n_step, kernels, device, pixel, frame_stacks)
        self.gamma = gamma
        n, N, D, A = self.n, self.n_step, self.D, self.A
        f = lambda *s: torch.zeros(*s, device=self.device)  # noqa: E731
        self.carry = {'obs': f(n, N, D), 'actions': f(n, N, A), 'rewards': f(n, N)}
        self.gpow = torch.tensor([pow(gamma, e) for e in range(N)], dtype=torch.float64, device=self.device)
        self.shapes = {'obs': (D,), 'obs_next': (D,), 'actions': (A,), 'rewards': (), 'dones': ()}
        if self.pixel is not None:
            self._camera_shapes(None)

    def _closes(self, t):
        return t >= self.n_step - 1

    def record(self, replay, actions, rewards, dones, obs_next, obs_reset=None, monitor=None, frames_next=None,
               frames_reset=None, copy_workgroups=0):
        """one step of all actors -> the number of transitions written (arguments as DeviceWindowRecorder.record)"""
        actions = self._step_rows(actions, self.A, 'actions')
        dones, rows, dev, t_host, rank_host = self._stage(rewards, dones, obs_next, obs_reset, frames_next, frames_reset)
        if self.pixel is not None and getattr(replay, 'frame_pool_on', False):
            # the frame-pool layout: every frame once in the replay's pool, which is the frame history as well
            low = {k: v for k, v in self.shapes.items() if k not in ('pixel', 'pixel_next')}
            h = self._pool_reserve(replay, dones, rank_host, rows, low)
            r = dict(h, t_host=t_host, rank_host=rank_host, rows=rows, cur_obs=self.cur_obs, actions=actions,
                     n_step=self.n_step, gpow=self.gpow, carry=self.carry, obs_pixel=self.obs_pixel, **dev)
            self.K.record_ddpg_pixel_pool_nstep_step(r, copy_workgroups=copy_workgroups, monitor=monitor)
            replay.commit_frame_pool(rows, self._pool['f'])
            self._moved(dones, monitor)
            return rows
        tables, cursor = self._ring(replay, rows, self.shapes)
        r = dict(dev, t_host=t_host, rank_host=rank_host, rows=rows, cur_obs=self.cur_obs, actions=actions,
                 n_step=self.n_step, gpow=self.gpow, carry=self.carry, tables=tables, cursor=cursor)
        if self.pixel is None:
            self.K.record_ddpg_nstep_step(r, monitor=monitor)
        else:
            self.K.record_ddpg_pixel_nstep_step(self._camera(r), copy_workgroups=copy_workgroups, monitor=monitor)
        replay.commit_ring(rows)
        self._moved(dones, monitor)
        return rows
