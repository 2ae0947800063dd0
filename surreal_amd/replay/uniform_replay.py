"""
UniformReplay (surreal/replay/uniform_replay.py:6-74): a ring buffer with an insert cursor
``_next_idx``; ``sample`` draws ``batch_size`` indices uniformly WITH replacement
(``random.randint(0, len - 1)`` each); ready when ``len > sampling_start_size``.
"""
import random

import numpy as np
import torch

from . import frame_pool as FP
from .base import Replay


class UniformReplay(Replay):
    def __init__(self, learner_config, env_config, session_config, index=0):
        super().__init__(learner_config=learner_config, env_config=env_config,
                         session_config=session_config, index=index)
        self._memory = []
        self.memory_size = self.learner_config.replay.memory_size
        self._next_idx = 0
        # device tier
        self._dev_len = 0
        self._dev_next = 0
        self._draws = 0
        self.seed = int(self.session_config.replay.get('seed', 0)) + 7919 * int(index)
        # the camera fields' layout: False -- stacked 'pixel' / 'pixel_next' tables; True -- the frame pool (frame_pool.py)
        self.frame_pool_on = bool(self.learner_config.replay.get('device_frame_pool', False))
        self.frame_pool = None                   # (created by the first reserve_frame_pool)

    # state_dict() / load_state_dict() (Replay): the tables, the ring cursor and length, the sampling stream's seed and
    # its Philox draw counter -- the next sample_batch draws what the saved replay would have drawn
    _state_cursors = ('_dev_len', '_dev_next', '_draws', 'seed')

    def _state_capacity(self):
        return self.memory_size

    # ---- host tier: the reference semantics ---------------------------------------------
    def insert(self, exp_dict):
        if self._next_idx >= len(self._memory):
            self._memory.append(exp_dict)
        else:
            self._memory[self._next_idx] = exp_dict
        self._next_idx = (self._next_idx + 1) % self.memory_size

    def sample(self, batch_size):
        indices = [random.randint(0, len(self._memory) - 1) for _ in range(batch_size)]
        return [self._memory[i] for i in indices]

    def evict(self):
        raise NotImplementedError

    def start_sample_condition(self):
        return len(self) > self.learner_config.replay.sampling_start_size

    def __len__(self):
        return len(self._memory) + self._dev_len

    # ---- device tier -----------------------------------------------------------------------
    def insert_batch(self, fields):
        if self.frame_pool_on:
            raise ValueError('insert_batch: a frame-pool replay (replay.device_frame_pool) stores raw frames once and '
                             'rows that name them; stacked rows carry no frame identities -- record through '
                             'reserve_frame_pool (ddpg_rollout_into, DeviceNStepRecorder)')
        tables = self._ensure_tables(self.memory_size, fields)
        n = next(iter(fields.values())).shape[0]
        if n > self.memory_size:
            fields = {k: v[n - self.memory_size:] for k, v in fields.items()}
            n = self.memory_size
        for name, t in fields.items():
            tables[name].insert(self._dev_next, t)
        self._dev_next = (self._dev_next + n) % self.memory_size
        self._dev_len = min(self.memory_size, self._dev_len + n)
        self.cumulative_collected_count += n

    def reserve_ring(self, rows, shapes, dtypes=None):
        """zero-copy insertion: -> (tables, cursor, capacity), tables = {field: [capacity, width] device table}
        (created here on first use, like insert_batch) for a producer that writes `rows` rows itself at
        (cursor + i) % capacity, i < rows; commit_ring(rows) then makes them part of the replay.  dtypes: {field:
        torch dtype} for the fields whose table is not fp32 (uint8 camera frames)"""
        if rows > self.memory_size:
            raise ValueError('reserve_ring: %d rows do not fit a ring of %d' % (rows, self.memory_size))
        if self.frame_pool_on and ('pixel' in shapes or 'pixel_next' in shapes):
            raise ValueError('reserve_ring: stacked pixel fields into a frame-pool replay; use reserve_frame_pool')
        dtypes = dict(dtypes or {})
        tables = self._ensure_tables(self.memory_size, {k: torch.empty((0,) + tuple(s), dtype=dtypes.get(k, torch.float32))
                                                        for k, s in shapes.items()})
        for k, s in shapes.items():
            if k not in tables or tables[k].shape != tuple(s) or tables[k].dtype != dtypes.get(k, torch.float32):
                raise ValueError('reserve_ring: field %r %s %s does not match the replay table'
                                 % (k, tuple(s), dtypes.get(k, torch.float32)))
        return {k: tables[k].data for k in shapes}, self._dev_next, self.memory_size

    def commit_ring(self, rows):
        """the `rows` rows written after reserve_ring: advance the cursor and the counters as insert_batch does"""
        self._dev_next = (self._dev_next + rows) % self.memory_size
        self._dev_len = min(self.memory_size, self._dev_len + rows)
        self.cumulative_collected_count += rows

    # ---- the frame-pool layout (replay.device_frame_pool; frame_pool.py) ---------------------------------------------
    def reserve_frame_pool(self, steps, shapes, n, frame_shape, frame_stacks, n_step):
        """reserve_ring for a producer of camera transitions in the frame-pool layout -> a dict: 'tables' (the
        low-dimensional fields of `shapes`), 'cursor', 'capacity', and the pool: 'pool' uint8 [n, P, F] (actor a's frame
        with counter i in slot i % P), 'frame_next' / 'frame_first' int64 [capacity], 'frame_actor' int32 [capacity],
        'counter' int64 [n] (numpy: each actor's newest counter, -1 before its first frame), 'frame_stacks', 'n_step'.
        steps: the call's recorded steps in order, [(rows the step closes, the counters after it -- a scalar on a shared
        clock, else [n] --, the oldest counter its rows name (frame_pool.oldest_frame; likewise))]: a step that writes
        frames and closes nothing has rows 0.  The rows whose frames the call overwrites are retired HERE, before the
        producer enqueues anything; commit_frame_pool makes the call's own rows part of the replay.
        P = replay.device_frame_pool_steps, by default ceil(memory_size / n) + n_step + frame_stacks"""
        if not self.frame_pool_on:
            raise ValueError('reserve_frame_pool: the replay keeps stacked tables (replay.device_frame_pool is off)')
        # (the steps are launches of their own: together they may go round the ring, one of them may not)
        tables, cursor, cap = self.reserve_ring(max([0] + [int(s[0]) for s in steps]), shapes)
        N, S, n = int(n_step), int(frame_stacks), int(n)
        F = int(np.prod(frame_shape))
        fp = self.frame_pool
        if fp is None:
            P = int(self.learner_config.replay.get('device_frame_pool_steps', 0)) or FP.default_pool_steps(cap, n, N, S)
            if P < N + S + 1:
                raise ValueError('replay.device_frame_pool_steps = %d: a pool holds at least n_step + frame_stacks + 1 '
                                 '= %d frames per actor' % (P, N + S + 1))
            dev = self._dev
            fp = self.frame_pool = dict(
                pool=torch.zeros(n, P, F, device=dev, dtype=torch.uint8),
                frame_next=torch.zeros(cap, device=dev, dtype=torch.int64),
                frame_first=torch.zeros(cap, device=dev, dtype=torch.int64),
                frame_actor=torch.zeros(cap, device=dev, dtype=torch.int32),
                counter=np.full(n, -1, dtype=np.int64), frame_stacks=S, n_step=N, frame_shape=tuple(frame_shape),
                ledger=FP.FramePoolLedger(cap, P))
        elif (tuple(fp['pool'].shape[::2]), fp['frame_stacks'], fp['n_step']) != ((n, F), S, N):
            raise ValueError('reserve_frame_pool: %d actors, frames of %d bytes, frame_stacks %d, n_step %d do not match '
                             'the replay\'s pool' % (n, F, S, N))
        old, fp['pending'] = fp['ledger'].plan(steps)
        self._dev_len = old
        return dict(fp, tables=tables, cursor=cursor, capacity=cap)

    def commit_frame_pool(self, rows, counter):
        """the producer has enqueued the call reserve_frame_pool planned: `rows` rows, the counters now `counter`"""
        fp = self.frame_pool
        self._dev_next = (self._dev_next + rows) % self.memory_size
        self._dev_len = fp.pop('pending')
        fp['counter'][:] = counter
        self.cumulative_collected_count += rows

    def camera_bytes(self):
        """device bytes of the camera fields: the stacked tables, or the pool and the rows' counters"""
        if self.frame_pool is not None:
            fp = self.frame_pool
            return sum(fp[k].numel() * fp[k].element_size() for k in ('pool', 'frame_next', 'frame_first', 'frame_actor'))
        return sum(t.data.numel() for k, t in (self._tables or {}).items() if k in ('pixel', 'pixel_next'))

    def _live_base(self):
        """the ring row of the oldest live row"""
        return (self._dev_next - self._dev_len) % self.memory_size

    def _sample_pool(self, batch_size, idx, out):
        """sample_batch in the frame-pool layout: ONE launch (smx_uniform_gather_pool)"""
        fp, cap = self.frame_pool, self.memory_size
        if fp is None:
            raise ValueError('sample_batch: nothing was recorded into the frame-pool replay yet')
        if idx is not None:
            # (injected rows must be live: their frames are gone otherwise; this reads the indices back -- parity tests)
            rows = idx.cpu().numpy()
            age = (self._dev_next - 1 - rows) % cap              # (0: the newest row)
            if rows.size != batch_size or bool(((rows < 0) | (rows >= cap) | (age >= self._dev_len)).any()):
                raise ValueError('sample_batch: an injected index is not a live row of the frame-pool replay (%d live '
                                 'rows behind cursor %d)' % (self._dev_len, self._dev_next))
        names = list(self._tables)
        assert len(names) <= 8, names
        tabs = [self._tables[k] for k in names]
        S, (C, H, W) = fp['frame_stacks'], fp['frame_shape']
        specs = [(k, t.width, t.dtype, t.shape) for k, t in zip(names, tabs)]
        specs += [(k, S * C * H * W, torch.uint8, (S * C, H, W)) for k in ('pixel', 'pixel_next')]
        outs = []
        for k, width, dtype, _ in specs:
            o = None if out is None else out.get(k)
            if o is None:
                o = torch.empty(batch_size, width, device=self._dev, dtype=dtype)
            else:
                assert (o.is_contiguous() and o.dtype == dtype and o.numel() == batch_size * width
                        and o.shape[0] == batch_size), k
                o = o.view(batch_size, width)
            outs.append(o)
        self._K.uniform_gather_pool([t.data for t in tabs], outs[:-2], fp, outs[-2], outs[-1], self._dev_len, self.seed,
                                    self._draws, self._live_base(), idx=idx)
        if idx is None:
            self._draws += batch_size
        return {k: o.view((batch_size,) + shape) for (k, _, _, shape), o in zip(specs, outs)}

    def sample_indices(self, batch_size):
        """with-replacement uniform indices on the device (Philox4x32-10; the reference's
        Python Mersenne stream cannot be reproduced on a GPU -- distributional parity, and
        sample_batch(indices=...) takes injected indices for exact-parity tests)"""
        idx = torch.empty(batch_size, dtype=torch.int64, device=self._dev)
        self._K.uniform_indices(idx, self._dev_len, self.seed, self._draws)
        self._draws += batch_size
        if self.frame_pool_on:                   # (a draw among the live rows: the newest _dev_len of the ring)
            idx = (idx + self._live_base()) % self.memory_size
        return idx

    def sample_batch(self, batch_size, indices=None, out=None):
        """one launch for the whole sample (smx_uniform_gather_multi): every field's rows, the indices drawn where they
        are used -- the same Philox counters as sample_indices(), so the two agree row for row.
        out: {field: tensor} to gather INTO (contiguous, the field's dtype, batch_size rows) -- e.g. a learner's staging
        buffers (DDPGLearner.staging_fields): the batch then needs no copy on its way into the captured iteration.
        A frame-pool replay (replay.device_frame_pool) returns the same dict, 'pixel' / 'pixel_next' built from the pool in
        the same launch (smx_uniform_gather_pool); the rows are drawn among the live ones, and an injected index that is
        not live is a ValueError"""
        idx = None if indices is None else torch.as_tensor(indices, dtype=torch.int64).to(self._dev)
        self.cumulative_sampled_count += batch_size
        if self.frame_pool_on:
            return self._sample_pool(batch_size, idx, out)
        names = list(self._tables)
        if len(names) > 8:                       # (more fields than one launch carries: field by field)
            idx = self.sample_indices(batch_size) if idx is None else idx
            return {name: tab.gather(idx) for name, tab in self._tables.items()}
        tabs = [self._tables[k] for k in names]
        outs = []
        for k, t in zip(names, tabs):
            o = None if out is None else out.get(k)
            if o is None:
                o = torch.empty(batch_size, t.width, device=self._dev, dtype=t.dtype)
            else:
                assert (o.is_contiguous() and o.dtype == t.dtype and o.numel() == batch_size * t.width
                        and o.shape[0] == batch_size), k
                o = o.view(batch_size, t.width)
            outs.append(o)
        self._K.uniform_gather_multi([t.data for t in tabs], outs, self._dev_len, self.seed, self._draws, idx=idx)
        if idx is None:
            self._draws += batch_size
        return {k: o.view((batch_size,) + t.shape) for k, o, t in zip(names, outs, tabs)}
