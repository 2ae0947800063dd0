"""Recording host-stepped environments (GPU box): per-step time of
  (a) the host path -- n experience wrappers stepped in actor order (ExpSenderWrapperMultiStepMovingWindowWithInfo /
      ExpSenderWrapperSSARNStepBootstrap over environments that only play back pre-made arrays), the experiences of the
      step stacked and put into the replay's device tables with insert_batch; `host_insert` is the same with the host
      tier's insert per experience instead (nothing reaches the device);
  (b) DeviceWindowRecorder / DeviceNStepRecorder.record() alone on the same stream as pre-made host arrays (actions and
      pds already on the device, as act_batch leaves them).
Every step is timed with the host clock around work that ends in a device synchronise; the two paths alternate in rounds
of `--steps` steps, each path going on with its own stream.  One JSON line per case: the median over all timed steps,
the per-round medians (the spread) and the ratio (b) / (a).
    python scripts/bench_record.py [--rounds 5] [--steps 60] [--warmup 25] [--out FILE]
    python scripts/bench_record.py --profile     # all-closing record() steps only, for rocprofv3 --kernel-trace --stats
With --pixel C H W --frame-stacks S the environments also emit one raw uint8 frame per step: (a) is then n host chains
env -> FrameStackWrapper (concatenate on env) -> experience wrapper with the stacked frames in insert_batch, (b) record()
with the camera (frames_next / frames_reset as host arrays: the frames cross the bus in the step's one copy).
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ddpg_rollout_cases as DC  # noqa: E402
import ppo_window_cases as PW  # noqa: E402
from surreal_amd.env import DeviceNStepRecorder, DeviceWindowRecorder  # noqa: E402
from surreal_amd.env import ExpSenderWrapperMultiStepMovingWindowWithInfo, ExpSenderWrapperSSARNStepBootstrap  # noqa: E402
from surreal_amd.env.base import Env, FrameStackWrapper  # noqa: E402
from surreal_amd.replay import FIFOReplay, UniformReplay  # noqa: E402
from surreal_amd.session import Config  # noqa: E402

D, A = 376, 17
WINDOW = (25, 20)
DDPG_N, GAMMA = 3, 0.99
LENGTHS = [100, 140, 180, 220]           # episode lengths, every actor from another rotation: the clocks diverge
HBM_COPY_BYTES_PER_S = 6.3e12            # the achievable copy rate DESIGN.md 3.8 quotes
CAMERA = None                            # ((C, H, W), frame_stacks) with --pixel
FRAME_POOL = False                       # --frame-pool


class PlaybackEnv(Env):
    """plays back rows of a pre-made observation table and reward vector: its own cost is an index and a dict"""

    def __init__(self, obs, rewards, lengths, rotation, frames=None):
        self.obs, self.rewards, self.lengths, self.rotation, self.frames = obs, rewards, lengths, rotation, frames
        self.i = self.episode = self.t = 0
        self.length = None

    def _observe(self):
        self.i = (self.i + 1) % self.obs.shape[0]
        obs = collections.OrderedDict(low_dim=collections.OrderedDict(flat_inputs=self.obs[self.i]))
        if self.frames is not None:
            obs['pixel'] = collections.OrderedDict(camera0=self.frames[self.i])
        return obs

    def _reset(self):
        self.length = self.lengths[(self.rotation + self.episode) % len(self.lengths)]
        self.episode += 1
        self.t = 0
        return self._observe(), {}

    def _step(self, action):
        self.t += 1
        return self._observe(), float(self.rewards[self.i]), self.t >= self.length, {}


def _envs(n, seed=0):
    rs = np.random.RandomState(seed)
    obs = rs.standard_normal((257, D)).astype(np.float32)
    rewards = rs.standard_normal(257).astype(np.float32)
    frames = rs.randint(0, 256, (257,) + CAMERA[0]).astype(np.uint8) if CAMERA else None
    return [PlaybackEnv(obs, rewards, LENGTHS, a, frames) for a in range(n)]


def _flat(o):
    return o['low_dim']['flat_inputs']


def _cam(o):
    return o['pixel']['camera0']


class HostPath(object):
    """(a): n wrappers and the insert of what they emit"""

    def __init__(self, algo, n, replay, lc, sc, device_insert):
        self.algo, self.n, self.replay, self.device_insert = algo, n, replay, device_insert
        self.sent = []
        wrap = ExpSenderWrapperMultiStepMovingWindowWithInfo if algo == 'ppo' else ExpSenderWrapperSSARNStepBootstrap
        envs = _envs(n)
        if CAMERA:
            stack = Config(frame_stacks=CAMERA[1], frame_stack_concatenate_on_env=True)
            envs = [FrameStackWrapper(env, stack) for env in envs]
        self.ws = [wrap(env, lc, sc, sink=self.sent.append) for env in envs]
        for w in self.ws:
            w.reset()
        rs = np.random.RandomState(1)
        self.actions = rs.uniform(-1, 1, (n, A)).astype(np.float32)
        self.pds = rs.standard_normal((n, 2 * A)).astype(np.float32)

    def step(self):
        ppo = self.algo == 'ppo'
        for a, w in enumerate(self.ws):
            action = (self.actions[a], [[], [self.pds[a]]]) if ppo else self.actions[a]
            if w.step(action)[2]:
                w.reset()
        x, self.sent[:] = list(self.sent), []
        if not x:
            return 0
        if not self.device_insert:
            for e in x:
                self.replay._insert_wrapper(e)
            return len(x)
        if ppo:
            f = {'obs': np.stack([np.stack([_flat(o) for o in e['obs']]) for e in x]),
                 'obs_next': np.stack([_flat(e['obs_next'])[None] for e in x]),
                 'actions': np.stack([np.stack(e['actions']) for e in x]),
                 'rewards': np.asarray([e['rewards'] for e in x], np.float32),
                 'dones': np.asarray([e['dones'] for e in x], np.float32),
                 'pds': np.stack([np.stack([p[0] for p in e['persistent_infos']]) for e in x])}
            if CAMERA:
                f['pixel'] = np.stack([np.stack([_cam(o) for o in e['obs']]) for e in x])
                f['pixel_next'] = np.stack([_cam(e['obs_next'])[None] for e in x])
        else:
            f = {'obs': np.stack([_flat(e['obs'][0]) for e in x]), 'obs_next': np.stack([_flat(e['obs'][1]) for e in x]),
                 'actions': np.stack([e['action'] for e in x]), 'rewards': np.asarray([e['reward'] for e in x], np.float32),
                 'dones': np.asarray([e['done'] for e in x], np.float32)}
            if CAMERA:
                f['pixel'] = np.stack([_cam(e['obs'][0]) for e in x])
                f['pixel_next'] = np.stack([_cam(e['obs'][1]) for e in x])
        self.replay.insert_batch({k: torch.from_numpy(v).cuda() for k, v in f.items()})
        return len(x)


class RecordPath(object):
    """(b): record() on the stream the same environments give, made before the clock starts"""
    RING = 32
    FRAME_RING = 8

    def __init__(self, algo, n, replay, steps):
        self.algo, self.n, self.replay = algo, n, replay
        envs = _envs(n)
        first = [e.reset()[0] for e in envs]
        camera = dict(pixel=CAMERA[0], frame_stacks=CAMERA[1]) if CAMERA else {}
        if CAMERA:
            # FRAME_RING steps of frames (84 x 84 x 3: 21 KB a frame), as pinned buffers like HostVecEnv's
            u8 = lambda: torch.zeros((self.FRAME_RING, n) + CAMERA[0], dtype=torch.uint8, pin_memory=True).numpy()  # noqa: E731
            self.frames_next, self.frames_reset = u8(), u8()
        first_frames = (np.stack([_cam(o) for o in first]),) if CAMERA else ()
        first = np.stack([_flat(o) for o in first])
        # the observations of RING steps, gone through again and again (their values do not matter to the clock); the
        # rewards and the dones -- which drive the recorder's clocks -- of every step
        self.obs_next = np.zeros((self.RING, n, D), np.float32)
        self.obs_reset = np.zeros((self.RING, n, D), np.float32)
        self.rewards = np.zeros((steps, n), np.float32)
        self.dones = np.zeros((steps, n), bool)
        for s in range(steps):
            for a, e in enumerate(envs):
                o, r, d, _ = e.step(None)
                self.obs_next[s % self.RING, a], self.rewards[s, a], self.dones[s, a] = _flat(o), r, d
                if CAMERA:
                    self.frames_next[s % self.FRAME_RING, a] = _cam(o)
                if d:
                    o = e.reset()[0]
                    self.obs_reset[s % self.RING, a] = _flat(o)
                    if CAMERA:
                        self.frames_reset[s % self.FRAME_RING, a] = _cam(o)
        self.rec = (DeviceWindowRecorder(n, D, A, *WINDOW, **camera) if algo == 'ppo' else
                    DeviceNStepRecorder(n, D, A, DDPG_N, GAMMA, **camera))
        self.rec.begin(first, *first_frames)
        self.actions = torch.rand(n, A, device='cuda') * 2 - 1
        self.pds = torch.randn(n, 2 * A, device='cuda')
        self.s = 0

    def step(self, all_closing=False):
        s = self.s
        self.s += 1
        if all_closing:                             # (the profile run: every actor closes on every step)
            self.rec.t[:] = self.rec.n_step - 1
        frames = dict(frames_next=self.frames_next[s % self.FRAME_RING],
                      frames_reset=self.frames_reset[s % self.FRAME_RING]) if CAMERA else {}
        if self.algo == 'ppo':
            return self.rec.record(self.replay, self.actions, self.pds, self.rewards[s], self.dones[s],
                                   self.obs_next[s % self.RING], self.obs_reset[s % self.RING], **frames)
        return self.rec.record(self.replay, self.actions, self.rewards[s], self.dones[s], self.obs_next[s % self.RING],
                               self.obs_reset[s % self.RING], **frames)


def _replay(algo, n, frame_pool=False):
    """frame_pool: the DDPG camera replay in the frame-pool layout (what record() writes into; insert_batch of stacked rows
    has no meaning there, so the host paths keep the stacked one)"""
    if algo == 'ppo':
        lc, ec, sc = PW.configs(D, A, *WINDOW, hidden=(300, 200), memory_size=4 * n)
        return FIFOReplay(lc, ec, sc), lc, sc
    lc, ec, sc = DC.configs(D, A, n, hidden=(300, 200), n_step=DDPG_N, gamma=GAMMA, memory_size=(16 if CAMERA else 64) * n,
                            folder='surreal_amd_bench_record')
    if frame_pool and CAMERA:
        lc.replay.device_frame_pool = True
    return UniformReplay(lc, ec, sc), lc, sc


def _timed_steps(step, k):
    ms, rows = [], 0
    for _ in range(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows += step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, rows


def moved_bytes(algo, rows, n=0):
    """what a record() launch reads plus what it writes for `rows` closing actors (the step's own low-dimensional inputs
    and ring slot, a few KB per actor, not counted); with a camera also the closing experiences' stacked frames and, for
    each of the n actors, the new frame into the history and the acting observation"""
    per = WINDOW[0] * (D + 3 * A + 2) * 4 + D * 4 if algo == 'ppo' else (2 * D + A + 2) * 4
    if CAMERA and FRAME_POOL and algo == 'ddpg':
        # (a row gains two counters and its actor; per actor the input frame read once and stored twice, the
        # observation's S - 1 older frames out of the pool)
        (C, H, W), S = CAMERA
        return 2 * per * rows + 20 * rows + n * (1 + 2 * S) * C * H * W
    if CAMERA:
        (C, H, W), S = CAMERA
        per += ((WINDOW[0] + 1) if algo == 'ppo' else 2) * S * C * H * W
        return 2 * per * rows + n * (1 + 2 * S) * C * H * W          # (the input frame is read once, stored twice)
    return 2 * per * rows


def bench(algo, n, rounds, steps, warmup):
    paths = {}
    # (with a camera path (a) is the device insert alone: the host tier's per-experience insert is not part of it)
    for name, device_insert in (('host_insert_batch', True),) + ((() if CAMERA else (('host_insert', False),))):
        replay, lc, sc = _replay(algo, n)
        paths[name] = HostPath(algo, n, replay, lc, sc, device_insert).step
    paths['record'] = RecordPath(algo, n, _replay(algo, n, FRAME_POOL)[0], warmup + rounds * steps).step
    for name, step in paths.items():
        _timed_steps(step, warmup)
    times = {k: [] for k in paths}
    medians = {k: [] for k in paths}
    rows = {k: 0 for k in paths}
    for _ in range(rounds):
        for name, step in paths.items():
            ms, r = _timed_steps(step, steps)
            times[name] += ms
            medians[name].append(statistics.median(ms))
            rows[name] += r
    assert len(set(rows.values())) == 1, rows                # the three paths wrote the same experiences
    med = {k: statistics.median(v) for k, v in times.items()}
    line = {'case': algo, 'n': n, 'D': D, 'A': A, 'n_step': WINDOW[0] if algo == 'ppo' else DDPG_N,
            'stride': WINDOW[1] if algo == 'ppo' else None, 'pixel': CAMERA[0] if CAMERA else None,
            'frame_stacks': CAMERA[1] if CAMERA else None, 'frame_pool': bool(FRAME_POOL and CAMERA and algo == 'ddpg'),
            'rounds': rounds, 'steps_per_round': steps,
            'experiences_per_step': rows['record'] / (rounds * steps),
            'step_ms_median': med, 'step_ms_round_medians': medians,
            'step_ms_max': {k: max(v) for k, v in times.items()},
            'record_over_host_insert_batch': med['record'] / med['host_insert_batch']}
    if 'host_insert' in med:
        line['record_over_host_insert'] = med['record'] / med['host_insert']
    print(json.dumps(line), flush=True)
    return line


def profile(n, steps=40, warmup=5):
    """record() steps on which EVERY actor closes (the clocks are forced): run under rocprofv3 --kernel-trace --stats,
    the kernel's average time over bytes_per_launch is the launch's bytes per second"""
    lines = []
    for algo in ('ppo', 'ddpg'):
        path = RecordPath(algo, n, _replay(algo, n, FRAME_POOL)[0], warmup + steps)
        ms, rows = _timed_steps(lambda: path.step(all_closing=True), warmup + steps)
        assert rows == n * (warmup + steps)
        b = moved_bytes(algo, n, n)
        lines.append({'case': 'profile_' + algo, 'n': n, 'steps': steps, 'pixel': CAMERA[0] if CAMERA else None,
                      'frame_stacks': CAMERA[1] if CAMERA else None, 'bytes_per_launch': b,
                      'least_us_at_hbm_copy_rate': b / HBM_COPY_BYTES_PER_S * 1e6,
                      'record_step_ms_median': statistics.median(ms[warmup:])})
        print(json.dumps(lines[-1]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=25)
    ap.add_argument('--sizes', type=int, nargs='*', default=[64, 1024])
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', action='store_true', help='all-closing record() steps only (for a kernel trace)')
    ap.add_argument('--pixel', type=int, nargs=3, metavar=('C', 'H', 'W'), default=None,
                    help='the environments also emit one raw uint8 frame per step')
    ap.add_argument('--frame-stacks', type=int, default=3)
    ap.add_argument('--frame-pool', action='store_true',
                    help='with --pixel: DDPG\'s record() writes into a frame-pool replay (replay.device_frame_pool)')
    args = ap.parse_args()
    global CAMERA, FRAME_POOL
    FRAME_POOL = bool(args.frame_pool)
    if args.pixel:
        CAMERA = (tuple(args.pixel), args.frame_stacks)
    if not torch.cuda.is_available():
        raise SystemExit('bench_record.py measures on the GPU: no device is visible')
    if args.profile:
        lines = [ln for n in args.sizes for ln in profile(n)]
    else:
        lines = [bench(algo, n, args.rounds, args.steps, args.warmup) for algo in ('ppo', 'ddpg') for n in args.sizes]
    if args.out:
        with open(args.out, 'w') as f:
            for ln in lines:
                f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
