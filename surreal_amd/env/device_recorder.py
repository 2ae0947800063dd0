"""
Recording the steps of n HOST-stepped environments (GymAdapter, DMControlAdapter, RobosuiteWrapper: simulators that end
their episodes whenever they like) into the replays' device rings: what n experience wrappers do per step on the host
(exp_sender_wrapper.py: a ring of n_step slots per actor, one ``insert`` per experience) as ONE launch per step for all
actors (csrc/smx_record.hip), every actor on an episode clock of its own.  Low-dimensional observations only.

The host keeps the clocks -- it sees the dones -- and per step computes who closes an experience and where it goes:

  PPO   actor a at step t of its episode closes window t + 1 - N iff that is >= 0 and a multiple of advance
  DDPG  actor a emits transition t - N + 1 iff t >= N - 1
  rank  the actor's position among this step's closing actors in ascending actor order (-1: none); its row is
        (cursor + rank) % capacity, so a step's rows are dense and in the order n host wrappers stepped in actor order
        would have inserted them.

What the device needs of a step travels in ONE pinned staging set -- clocks, ranks, dones and whichever of rewards /
obs_next / obs_reset are host arrays -- by one copy.  There are two sets, each with an event recorded behind its copy
that is waited on before the host writes the set again; nothing else synchronises.
"""
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
    obs_reset (fp32 [n, D]); the host side as numpy views, the device side as tensors"""
    FIELDS = ('t', 'rank', 'dones', 'rewards', 'obs_next', 'obs_reset')

    def __init__(self, n, D, device):
        cuda = device.type == 'cuda'
        sizes = (n, n, n, n, n * D, n * D)
        self.host = torch.zeros(sum(_pad4(s) for s in sizes), dtype=torch.int32, pin_memory=cuda)
        self.dev = torch.zeros(self.host.numel(), dtype=torch.int32, device=device)
        self.event = torch.cuda.Event() if cuda else None
        self.in_flight = False
        words = self.host.numpy()
        self.h, self.d, self.end = {}, {}, {}
        off = 0
        for name, size in zip(self.FIELDS, sizes):
            h, d = words[off:off + size], self.dev[off:off + size]
            if name not in ('t', 'rank'):
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
    """what the two recorders share: the clocks, cur_obs, the staging sets"""

    def __init__(self, n, D, A, n_step, kernels=None, device=None):
        self.n, self.D, self.A, self.n_step = int(n), int(D), int(A), int(n_step)
        if min(self.n, self.D, self.A, self.n_step) < 1:
            raise ValueError('recorder: n, D, A and n_step must be positive, got %r' % ((n, D, A, n_step),))
        self.K = kernels if kernels is not None else KN.default_kernels()
        self.device = torch.device(device if device is not None else KN.default_device())
        self.cur_obs = torch.zeros(self.n, self.D, device=self.device)
        self.t = np.zeros(self.n, dtype=np.int32)            # each actor's step within its episode
        self.carry = {}
        self._sets = [_StagingSet(self.n, self.D, self.device) for _ in range(2)]
        self._next = 0

    @property
    def observation(self):
        """[n, D] on the device: what every actor acts on next (act_batch reads it; record() moves it on)"""
        return self.cur_obs

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

    def begin(self, obs):
        """the first observations [n, D] of n fresh episodes; all clocks to 0"""
        self.cur_obs.copy_(self._device_rows(obs, self.D))
        self.t[:] = 0

    def reset(self, mask=None, obs=None):
        """restart the episodes of the actors in `mask` (host bool [n]; None: all) outside record() -- their clocks go to
        0 and their open windows / transitions are dropped; obs [n, D]: their first observations (the masked rows)"""
        mask = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(self.n)
        self.t[mask] = 0
        if obs is not None:
            m = torch.as_tensor(mask).to(self.device)
            self.cur_obs.copy_(torch.where(m.view(-1, 1), self._device_rows(obs, self.D), self.cur_obs))

    def state_dict(self):
        return {'t': self.t.copy(), 'cur_obs': self.cur_obs.detach().cpu().clone(),
                'carry': {k: v.detach().cpu().clone() for k, v in self.carry.items()}}

    def load_state_dict(self, sd):
        if set(sd['carry']) != set(self.carry):
            raise ValueError('recorder: the state holds rings %s, this recorder %s'
                             % (sorted(sd['carry']), sorted(self.carry)))
        self.t[:] = np.asarray(sd['t'], dtype=np.int32).reshape(self.n)
        self.cur_obs.copy_(self._device_rows(sd['cur_obs'], self.D))
        for k, v in self.carry.items():
            v.copy_(torch.as_tensor(sd['carry'][k]).reshape(v.shape))

    # ---- one step -------------------------------------------------------------------------------------------------
    def _closes(self, t):
        raise NotImplementedError

    def _stage(self, rewards, dones, obs_next, obs_reset):
        """this step's clocks, ranks, dones and host arrays into the next staging set and on their way ->
        (dones bool [n], rows, {name: device tensor} for the launch, the set's host t / rank)"""
        n, D = self.n, self.D
        dones = np.asarray(dones).astype(bool).reshape(n)
        if obs_reset is None and dones.any():
            raise ValueError('record: actors %s are done and there is no obs_reset to go on from'
                             % np.flatnonzero(dones).tolist())
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
        s.upload(last)
        return dones, rows, dev, s.h['t'], s.h['rank']

    def _step_rows(self, x, width, name):
        if not self._on_device(x) or x.numel() != self.n * width:
            raise ValueError('record: %s must be a device tensor of %d x %d values' % (name, self.n, width))
        return x.to(torch.float32).contiguous()

    def _ring(self, replay, rows, shapes):
        tables, cursor, cap = replay.reserve_ring(rows, shapes)
        if self.n > cap:
            raise ValueError('record: %d actors exceed the replay ring of %d rows (all of them may close in one step)'
                             % (self.n, cap))
        return tables, cursor

    def _advance(self, dones):
        self.t = np.where(dones, 0, self.t + 1).astype(np.int32)


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
    """

    def __init__(self, n, D, A, n_step, stride, rnn_hidden=0, kernels=None, device=None):
        super().__init__(n, D, A, n_step, kernels, device)
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

    def _closes(self, t):
        start = t + 1 - self.n_step
        return (start >= 0) & (start % self.advance == 0)

    def record(self, replay, actions, pds, rewards, dones, obs_next, obs_reset=None, cells_before=None, monitor=None,
               copy_workgroups=0):
        """one step of all actors -> the number of windows written.  actions [n, A] / pds [n, 2A]: device tensors (what
        act_batch returned for `observation`); dones: host bool [n]; rewards [n], obs_next [n, D] (the terminal
        observation where done), obs_reset [n, D] (the first observation of the next episode: only the rows of done
        actors are read; required when any actor is done): host arrays or device tensors; cells_before: (h, c), each
        [n, rnn_hidden] (or [1, n, rnn_hidden]) on the device -- the LSTM state the step started from
        (PPOAgent.batch_cells_before); monitor: a DeviceEpisodeMonitor over the n actors.  Steps that close nothing
        still launch: the rings and `observation` move."""
        n, Hl = self.n, self.rnn_hidden
        if (cells_before is None) != (Hl == 0):
            raise ValueError('record: cells_before goes with rnn_hidden (%d)' % Hl)
        actions, pds = self._step_rows(actions, self.A, 'actions'), self._step_rows(pds, 2 * self.A, 'pds')
        hb = cb = None
        if Hl:
            hb, cb = (self._step_rows(x, Hl, 'cells_before') for x in cells_before)
        dones, rows, dev, t_host, rank_host = self._stage(rewards, dones, obs_next, obs_reset)
        tables, cursor = self._ring(replay, rows, self.shapes)
        self.K.record_ppo_window_step(
            dict(dev, t_host=t_host, rank_host=rank_host, rows=rows, cur_obs=self.cur_obs, actions=actions, pds=pds,
                 h_before=hb, c_before=cb, n_step=self.n_step, advance=self.advance, carry=self.carry, tables=tables,
                 cursor=cursor), copy_workgroups=copy_workgroups, monitor=monitor)
        replay.commit_ring(rows)
        if monitor is not None:
            monitor.count_steps(1)
        self._advance(dones)
        return rows


class DeviceNStepRecorder(_DeviceRecorder):
    """DDPG's n-step transitions (ExpSenderWrapperSSARNStepBootstrap, its fill-up discount exponents included) of n
    host-stepped actors, written into the uniform replay's device ring in SyntheticVecEnv.ddpg_rollout_into's layout: obs /
    obs_next [D], actions [A], rewards, dones.  The reward is the wrapper's fp64 sum in step order, rounded once."""

    def __init__(self, n, D, A, n_step, gamma, kernels=None, device=None):
        super().__init__(n, D, A, n_step, kernels, device)
        self.gamma = gamma
        n, N, D, A = self.n, self.n_step, self.D, self.A
        f = lambda *s: torch.zeros(*s, device=self.device)  # noqa: E731
        self.carry = {'obs': f(n, N, D), 'actions': f(n, N, A), 'rewards': f(n, N)}
        self.gpow = torch.tensor([pow(gamma, e) for e in range(N)], dtype=torch.float64, device=self.device)
        self.shapes = {'obs': (D,), 'obs_next': (D,), 'actions': (A,), 'rewards': (), 'dones': ()}

    def _closes(self, t):
        return t >= self.n_step - 1

    def record(self, replay, actions, rewards, dones, obs_next, obs_reset=None, monitor=None):
        """one step of all actors -> the number of transitions written (arguments as DeviceWindowRecorder.record)"""
        actions = self._step_rows(actions, self.A, 'actions')
        dones, rows, dev, t_host, rank_host = self._stage(rewards, dones, obs_next, obs_reset)
        tables, cursor = self._ring(replay, rows, self.shapes)
        self.K.record_ddpg_nstep_step(
            dict(dev, t_host=t_host, rank_host=rank_host, rows=rows, cur_obs=self.cur_obs, actions=actions,
                 n_step=self.n_step, gpow=self.gpow, carry=self.carry, tables=tables, cursor=cursor), monitor=monitor)
        replay.commit_ring(rows)
        if monitor is not None:
            monitor.count_steps(1)
        self._advance(dones)
        return rows
