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
from surreal_amd.env.base import Env  # noqa: E402
from surreal_amd.replay import FIFOReplay, UniformReplay  # noqa: E402

D, A = 376, 17
WINDOW = (25, 20)
DDPG_N, GAMMA = 3, 0.99
LENGTHS = [100, 140, 180, 220]           # episode lengths, every actor from another rotation: the clocks diverge
HBM_COPY_BYTES_PER_S = 6.3e12            # the achievable copy rate DESIGN.md 3.8 quotes


class PlaybackEnv(Env):
    """plays back rows of a pre-made observation table and reward vector: its own cost is an index and a dict"""

    def __init__(self, obs, rewards, lengths, rotation):
        self.obs, self.rewards, self.lengths, self.rotation = obs, rewards, lengths, rotation
        self.i = self.episode = self.t = 0
        self.length = None

    def _observe(self):
        self.i = (self.i + 1) % self.obs.shape[0]
        return collections.OrderedDict(low_dim=collections.OrderedDict(flat_inputs=self.obs[self.i]))

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
    return [PlaybackEnv(obs, rewards, LENGTHS, a) for a in range(n)]


def _flat(o):
    return o['low_dim']['flat_inputs']


class HostPath(object):
    """(a): n wrappers and the insert of what they emit"""

    def __init__(self, algo, n, replay, lc, sc, device_insert):
        self.algo, self.n, self.replay, self.device_insert = algo, n, replay, device_insert
        self.sent = []
        wrap = ExpSenderWrapperMultiStepMovingWindowWithInfo if algo == 'ppo' else ExpSenderWrapperSSARNStepBootstrap
        self.ws = [wrap(env, lc, sc, sink=self.sent.append) for env in _envs(n)]
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
        else:
            f = {'obs': np.stack([_flat(e['obs'][0]) for e in x]), 'obs_next': np.stack([_flat(e['obs'][1]) for e in x]),
                 'actions': np.stack([e['action'] for e in x]), 'rewards': np.asarray([e['reward'] for e in x], np.float32),
                 'dones': np.asarray([e['done'] for e in x], np.float32)}
        self.replay.insert_batch({k: torch.from_numpy(v).cuda() for k, v in f.items()})
        return len(x)


class RecordPath(object):
    """(b): record() on the stream the same environments give, made before the clock starts"""
    RING = 32

    def __init__(self, algo, n, replay, steps):
        self.algo, self.n, self.replay = algo, n, replay
        envs = _envs(n)
        first = np.stack([_flat(e.reset()[0]) for e in envs])
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
                if d:
                    self.obs_reset[s % self.RING, a] = _flat(e.reset()[0])
        self.rec = DeviceWindowRecorder(n, D, A, *WINDOW) if algo == 'ppo' else DeviceNStepRecorder(n, D, A, DDPG_N, GAMMA)
        self.rec.begin(first)
        self.actions = torch.rand(n, A, device='cuda') * 2 - 1
        self.pds = torch.randn(n, 2 * A, device='cuda')
        self.s = 0

    def step(self, all_closing=False):
        s = self.s
        self.s += 1
        if all_closing:                             # (the profile run: every actor closes on every step)
            self.rec.t[:] = self.rec.n_step - 1
        if self.algo == 'ppo':
            return self.rec.record(self.replay, self.actions, self.pds, self.rewards[s], self.dones[s],
                                   self.obs_next[s % self.RING], self.obs_reset[s % self.RING])
        return self.rec.record(self.replay, self.actions, self.rewards[s], self.dones[s], self.obs_next[s % self.RING],
                               self.obs_reset[s % self.RING])


def _replay(algo, n):
    if algo == 'ppo':
        lc, ec, sc = PW.configs(D, A, *WINDOW, hidden=(300, 200), memory_size=4 * n)
        return FIFOReplay(lc, ec, sc), lc, sc
    lc, ec, sc = DC.configs(D, A, n, hidden=(300, 200), n_step=DDPG_N, gamma=GAMMA, memory_size=64 * n,
                            folder='surreal_amd_bench_record')
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


def moved_bytes(algo, rows):
    """what a record() launch reads plus what it writes for `rows` closing actors (the step's own inputs and ring slot,
    a few KB per actor, not counted)"""
    per = WINDOW[0] * (D + 3 * A + 2) * 4 + D * 4 if algo == 'ppo' else (2 * D + A + 2) * 4
    return 2 * per * rows


def bench(algo, n, rounds, steps, warmup):
    paths = {}
    for name, device_insert in (('host_insert_batch', True), ('host_insert', False)):
        replay, lc, sc = _replay(algo, n)
        paths[name] = HostPath(algo, n, replay, lc, sc, device_insert).step
    paths['record'] = RecordPath(algo, n, _replay(algo, n)[0], warmup + rounds * steps).step
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
            'stride': WINDOW[1] if algo == 'ppo' else None, 'rounds': rounds, 'steps_per_round': steps,
            'experiences_per_step': rows['record'] / (rounds * steps),
            'step_ms_median': med, 'step_ms_round_medians': medians,
            'step_ms_max': {k: max(v) for k, v in times.items()},
            'record_over_host_insert_batch': med['record'] / med['host_insert_batch'],
            'record_over_host_insert': med['record'] / med['host_insert']}
    print(json.dumps(line), flush=True)
    return line


def profile(n, steps=40, warmup=5):
    """record() steps on which EVERY actor closes (the clocks are forced): run under rocprofv3 --kernel-trace --stats,
    the kernel's average time over bytes_per_launch is the launch's bytes per second"""
    lines = []
    for algo in ('ppo', 'ddpg'):
        path = RecordPath(algo, n, _replay(algo, n)[0], warmup + steps)
        ms, rows = _timed_steps(lambda: path.step(all_closing=True), warmup + steps)
        assert rows == n * (warmup + steps)
        b = moved_bytes(algo, n)
        lines.append({'case': 'profile_' + algo, 'n': n, 'steps': steps, 'bytes_per_launch': b,
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
    args = ap.parse_args()
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
