"""LSTM-stem PPO rollouts (GPU box): the per-step stem path (_rollout_stem: act_batch + step launch per step) against
the one-launch kernel (smx_synth_lstm_rollout_f32), timed alternately in one process with device events after warm-up.
One JSON line per shape: median / min / max ms per rollout of each path over the repetitions.
    python scripts/bench_lstm_rollout.py [--reps 7] [--out FILE] [--device-noise]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import lstm_rollout_cases as LC  # noqa: E402
from surreal_amd.env import SyntheticVecEnv  # noqa: E402

SHAPES = [  # n, T, D, A, (H1, H2), rnn_hidden
    (1024, 128, 376, 17, (300, 200), 100),
    (64, 128, 17, 6, (300, 200), 100),
    (1024, 128, 17, 6, (300, 200), 100),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--device-noise', action='store_true',
                    help='draw the exploration noise inside the launches from the env\'s Philox stream (attach_noise): no '
                         'eps tensor; the stem path gets the same numbers from the fill kernel')
    args = ap.parse_args()
    lines = []
    for n, T, D, A, hidden, H in SHAPES:
        agent, _ = LC.make_agent(D, A, hidden=hidden, rnn_hidden=H, T=T, n=n)
        venv = SyntheticVecEnv(n, D, A, episode_len=T)
        eps = None if args.device_noise else torch.randn(T, n, A, device='cuda')
        if args.device_noise:
            venv.attach_noise(seed=1)
        times = {'stem': [], 'one_launch': []}

        def once(persistent):
            venv.reset()
            venv.persistent = persistent
            venv.start_rollout(T, info_width=2 * A)
            venv.rollout(agent, eps=eps)
        for _ in range(args.warmup):
            once(False)
            once(True)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, persistent in (('stem', False), ('one_launch', True)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                once(persistent)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        rec = {'n': n, 'T': T, 'D': D, 'A': A, 'hidden': list(hidden), 'rnn_hidden': H, 'reps': args.reps,
               'device_noise': bool(args.device_noise)}
        for name, v in times.items():
            v = sorted(v)
            rec[name + '_ms'] = {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}
        rec['speedup_median'] = rec['stem_ms']['median'] / rec['one_launch_ms']['median']
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
