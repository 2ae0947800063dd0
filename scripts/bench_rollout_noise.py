"""What the exploration noise costs the device rollouts (GPU box): each of rollout (376 -> 300 -> 200 -> 17), the LSTM 100
rollout, ppo_rollout_into at (25, 20) and ddpg_rollout_into at 1024 actors x 128 steps, called as a user calls it
(eps=None), once with the default draws (torch.randn + launch) and once with the env's Philox stream attached
(attach_noise: the draws are formed inside the launch).  Rounds interleave the variants; one JSON line per workload,
variant and round: the median ms of `calls` calls (device events around each call).  On a tree without attach_noise only
the default variant runs -- the same script times the commit before the stream.
    python scripts/bench_rollout_noise.py [--rounds 5] [--calls 12] [--tag NAME] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import ddpg_rollout_cases as DC  # noqa: E402
import lstm_rollout_cases as LC  # noqa: E402
import ppo_window_cases as PW  # noqa: E402
from surreal_amd.env import SyntheticVecEnv  # noqa: E402
from surreal_amd.replay import FIFOReplay, UniformReplay  # noqa: E402

N, T = 1024, 128


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def workloads(stream):
    """-> {name: a function that makes one call}; stream: attach the Philox stream to every env"""
    def env(D, A, L):
        venv = SyntheticVecEnv(N, D, A, episode_len=L)
        if stream:
            venv.attach_noise(seed=1)
        return venv
    out = {}
    agent, _ = PW.make_agent(376, 17, 25, 20, hidden=(300, 200))
    tab = env(376, 17, T)
    tab.start_rollout(T, info_width=34)

    def rollout(venv=tab, agent=agent):
        venv.reset()
        venv.slot = 0
        agent._batch_cells = None
        venv.rollout(agent)
    out['rollout'] = rollout
    lagent, _ = LC.make_agent(17, 6, hidden=(300, 200), rnn_hidden=100, T=T, n=N)
    ltab = env(17, 6, T)
    ltab.start_rollout(T, info_width=12)
    out['lstm_rollout'] = lambda: rollout(ltab, lagent)
    wagent, cfg = PW.make_agent(376, 17, 25, 20, hidden=(300, 200), memory_size=N * (T // 20 + 2))
    replay = FIFOReplay(*cfg)
    win = env(376, 17, 1000)

    def window():
        win.ppo_rollout_into(wagent, replay, T)
        while len(replay):
            replay.sample_batch(min(len(replay), replay.memory_size), copy=False)
    out['ppo_rollout_into'] = window
    lc, ec, sc = DC.configs(17, 6, N, hidden=(300, 200), noise_type='ou_noise', memory_size=1000000)
    dagent = DC.make_agent(lc, ec, sc, w3_scale=1.0)
    ring = UniformReplay(lc, ec, sc)
    denv = env(17, 6, 1000)
    out['ddpg_rollout_into'] = lambda: denv.ddpg_rollout_into(dagent, ring, T)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=12)
    ap.add_argument('--tag', default='this')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    variants = {'default': workloads(False)}
    if hasattr(SyntheticVecEnv, 'attach_noise'):
        variants['stream'] = workloads(True)
    for w in variants.values():
        for fn in w.values():
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    lines = []
    for r in range(args.rounds):
        for name in variants['default']:
            for v, w in variants.items():
                ms = [_timed(w[name]) for _ in range(args.calls)]
                lines.append({'tree': args.tag, 'workload': name, 'variant': v, 'round': r, 'actors': N, 'steps': T,
                              'calls': args.calls, 'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)})
                print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            for ln in lines:
                f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
