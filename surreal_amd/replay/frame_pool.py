"""
The frame-pool layout of the device uniform replay's camera fields (include/surreal_amd.h, above
smx_synth_ddpg_pixel_pool_step): every raw frame once in a per-actor pool of P slots, two counters per ring row in place
of the stacked 'pixel' / 'pixel_next'.  What the reference's pixel DDPG configuration does on the wire with
``frame_stack_concatenate_on_env: False`` (surreal/main/ddpg_configs.py:119-122; the learner joins the frames,
surreal/learner/ddpg.py:430-440).

``FramePoolLedger`` is the host's account of which ring rows may still be sampled: a row is live while the oldest frame
it names has not been overwritten.  Rows enter the ring in time order and the rows of one recorded step retire together,
so the live rows are the newest ``live`` rows of the ring; the ledger keeps one entry per recorded step that closed rows
-- no read-back, no atomics.
"""
import collections

import numpy as np


def default_pool_steps(memory_size, n, n_step, frame_stacks):
    """P = ceil(memory_size / n) + N + S: the frames of as many steps as fill the ring once, and a row's own reach.  (The
    first N - 1 steps of an episode write frames and close no rows, so with short episodes the live rows stay a little
    under memory_size.)"""
    return -(-int(memory_size) // int(n)) + int(n_step) + int(frame_stacks)


def oldest_frame(frame_next, frame_first, n_step, frame_stacks):
    """the oldest counter a row names: pixel's first frame, clamped at the episode's reset frame"""
    return np.maximum(frame_first, frame_next - n_step - frame_stacks + 1)


class FramePoolLedger(object):
    def __init__(self, capacity, pool_steps):
        self.capacity, self.P = int(capacity), int(pool_steps)
        self.live = 0
        self._steps = collections.deque()          # [rows, oldest counter(s) the step's rows name], oldest step first

    def retire(self, counter_after):
        """before the launch that moves the counters to `counter_after` (a scalar on a shared clock, else [n]) is
        enqueued: the steps with a row that names a frame older than counter_after - P + 1 leave, oldest first"""
        lo = np.asarray(counter_after, dtype=np.int64) - self.P + 1
        while self._steps and bool(np.any(self._steps[0][1] < lo)):
            self.live -= self._steps.popleft()[0]
        return self.live

    def add(self, rows, oldest):
        """a recorded step closed `rows` rows whose oldest frames are `oldest` (scalar, or [n] with a large value for
        the actors that closed none); rows pushed out of the ring leave"""
        if rows <= 0:
            return self.live
        self._steps.append([int(rows), np.asarray(oldest, dtype=np.int64)])
        self.live += int(rows)
        while self.live > self.capacity:
            over = self.live - self.capacity
            head = self._steps[0]
            cut = min(over, head[0])
            head[0] -= cut
            self.live -= cut
            if head[0] == 0:
                self._steps.popleft()
        return self.live

    def plan(self, steps):
        """a producer's call, step by step: steps = [(rows, counter_after, oldest)] -> (how many of the rows live before
        the call survive it, the live rows after it)"""
        added = 0
        for rows, counter_after, oldest in steps:
            self.retire(counter_after)
            self.add(rows, oldest)
            added += max(int(rows), 0)
        # (rows leave oldest first: whatever left beyond the call's own rows was there before it)
        return max(0, self.live - added), self.live
