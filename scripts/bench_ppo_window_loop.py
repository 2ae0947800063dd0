"""PPO moving-window rollouts (GPU box): SyntheticVecEnv.ppo_rollout_into (one launch that resumes mid-episode and writes
every closing window into the FIFO) against rollout() of the same T (an episode-boundary rollout into [n, T + 1]
tables, no windows), timed alternately in one process with device events after warm-up; then the loop at BASELINE
configs[1]'s shape (64 actors, 128-step chunks of 1000-step episodes, the reference-default algo config): chunk ->
ppo_rollout_into -> FIFOReplay.sample_batch(copy=False) -> PPOLearner.learn per batch.
One JSON line per case: median / min / max over the repetitions.
    python scripts/bench_ppo_window_loop.py [--reps 7] [--warmup 2] [--out FILE] [--quick]
--task drift|reach [--random-resets] --calls N: instead, N single ppo_rollout_into calls (plain MLP 300 / 200, windows of 25
steps 20 apart) on that task's dynamics at obs-dim 3 x action-dim, each between its own pair of events; one JSON line
with their median.
    python scripts/bench_ppo_window_loop.py --task reach --random-resets --calls 60 --actors 1024 --steps 128 \
        --action-dim 6 --episode-len 16"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import ppo_window_cases as PW  # noqa: E402
from surreal_amd.env import SyntheticVecEnv  # noqa: E402
from surreal_amd.replay import FIFOReplay  # noqa: E402

ROLLOUTS = [  # n, T, D, A, (H1, H2), rnn_hidden, (n_step, stride), episode_len
    (1024, 128, 376, 17, (300, 200), None, (10, 10), 1000),
    (1024, 128, 376, 17, (300, 200), None, (25, 20), 1000),
    (1024, 128, 17, 6, (300, 200), 100, (25, 20), 1000),
]


def _stats(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs)}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_rollouts(reps, warmup, shapes, monitor=False, device_noise=False, episode_lens=None):
    """episode_lens (LO, HI): an episode clock per actor for ppo_rollout_into, actor a with episodes of
    LO + a % (HI - LO + 1) steps; the table rollout next to it keeps the shared clock"""
    lines = []
    for n, T, D, A, hidden, H, (N, stride), L in shapes:
        own = None
        if episode_lens:
            lo, hi = episode_lens
            own = [lo + a % (hi - lo + 1) for a in range(n)]
        agent, cfg = PW.make_agent(D, A, N, stride, hidden=hidden, rnn_hidden=H, memory_size=n * (T // min(N, stride)
                                                                                                  + 2))
        replay = FIFOReplay(*cfg)
        win = SyntheticVecEnv(n, D, A, episode_len=own or L)
        tab = SyntheticVecEnv(n, D, A, episode_len=L)
        mon = win.attach_monitor() if monitor else None
        tab.start_rollout(T, info_width=2 * A)
        eps = None if device_noise else torch.randn(T, n, A, device='cuda')
        if device_noise:
            win.attach_noise(seed=1)
            tab.attach_noise(seed=1)
        times = {'window': [], 'rollout': []}
        rows = []

        def window():
            rows.append(win.ppo_rollout_into(agent, replay, T, eps=eps))

        def table():
            tab.reset()
            tab.slot = 0
            agent._batch_cells = None
            tab.rollout(agent, eps=eps)

        for r in range(warmup + reps):
            for name, fn in (('window', window), ('rollout', table)):
                ms = _timed(fn)
                if r >= warmup:
                    times[name].append(ms)
            while len(replay):                    # (the learner's pops: views, no launch)
                replay.sample_batch(min(len(replay), replay.memory_size), copy=False)
        w, t = _stats(times['window']), _stats(times['rollout'])
        lines.append({'case': 'rollout', 'n': n, 'T': T, 'D': D, 'A': A, 'hidden': list(hidden), 'rnn_hidden': H,
                      'n_step': N, 'stride': stride, 'episode_len': L, 'episode_lens': list(episode_lens or ()) or None,
                      'reps': reps, 'device_noise': device_noise, 'windows_per_call': sorted(set(rows)),
                      'ppo_rollout_into_ms': w, 'rollout_ms': t, 'ratio_median': w['median'] / t['median']})
        if mon is not None:
            mon.poll()
            lines[-1].update(mean_episode_return=mon.mean_reward(last=10), episodes=mon.num_episodes)
        print(json.dumps(lines[-1]), flush=True)
    return lines


def bench_loop(reps, warmup, n=64, T=128, L=1000, D=17, A=6, monitor=False, device_noise=False):
    """configs[1]'s shape with the reference-default algo config: env-steps/s of chunk -> FIFO -> learn"""
    from surreal_amd.learner import PPOLearner
    agent, cfg = PW.make_agent(D, A, 25, 20, hidden=(300, 200), rnn_hidden=100, memory_size=8 * n, batch_size=64)
    lc, ec, sc = cfg
    learner = PPOLearner(lc, ec, sc)
    agent.attach_learner(learner)
    agent.fetch_parameter()
    replay = FIFOReplay(lc, ec, sc)
    venv = SyntheticVecEnv(n, D, A, episode_len=L)
    mon = venv.attach_monitor() if monitor else None
    if device_noise:
        venv.attach_noise(seed=1)
    learned = [0]

    def chunk():
        venv.ppo_rollout_into(agent, replay, T)
        while len(replay) >= lc.replay.batch_size:
            learner.learn(venv.to_batch(replay.sample_batch(lc.replay.batch_size, copy=False)))
            learned[0] += lc.replay.batch_size
        agent.fetch_parameter()

    times = []
    for r in range(warmup + reps):
        ms = _timed(chunk)
        if r >= warmup:
            times.append(ms)
    s = _stats(times)
    line = {'case': 'loop', 'n': n, 'T': T, 'episode_len': L, 'D': D, 'A': A, 'n_step': 25, 'stride': 20,
            'rnn_hidden': 100, 'horizon': lc.algo.rnn.horizon, 'reps': reps, 'device_noise': device_noise, 'chunk_ms': s,
            'env_steps_per_s': {'at_median': n * T / (s['median'] * 1e-3), 'at_min_ms': n * T / (s['min'] * 1e-3),
                                'at_max_ms': n * T / (s['max'] * 1e-3)}, 'windows_learned': learned[0]}
    if mon is not None:
        mon.poll()
        line.update(mean_episode_return=mon.mean_reward(last=10), episodes=mon.num_episodes)
    print(json.dumps(line), flush=True)
    return [line]


def bench_task_calls(args):
    """--task: single calls of the one-launch windowed rollout on a task's dynamics"""
    n, T, A, L = args.actors, args.steps, args.action_dim, args.episode_len
    D, N, stride = (2 * A + 2 if args.task == 'arm' or args.arm_shape else 3 * A), 25, 20
    if L < N:                                       # (a window never crosses an episode end)
        N, stride = min(N, L), min(stride, L)
    agent, cfg = PW.make_agent(D, A, N, stride, hidden=(300, 200), rnn_hidden=None, memory_size=n * (T // min(N, stride) + 2))
    replay = FIFOReplay(*cfg)
    task = {'task': args.task} if args.task in ('reach', 'arm') else {}  # ('drift': no keyword, as before there were tasks)
    venv = SyntheticVecEnv(n, D, A, episode_len=L, **task)
    venv.attach_noise(seed=1)
    if args.random_resets:
        venv.attach_resets(seed=3, disturbance=args.disturbance)
        venv.reset()

    def call():
        venv.ppo_rollout_into(agent, replay, T)
        while len(replay):                          # (the learner's pops: views, no launch)
            replay.sample_batch(min(len(replay), replay.memory_size), copy=False)
    for _ in range(3):
        call()
    ms = sorted(_timed(call) for _ in range(args.calls))
    line = {'what': 'ppo_window_rollout_calls', 'label': args.label, 'task': args.task, 'random_resets': args.random_resets, 'disturbance': args.disturbance,
            'actors': n, 'steps': T, 'shape': [D, 300, 200, A], 'n_step': N, 'stride': stride, 'episode_len': L,
            'calls': args.calls, 'median_ms': round(ms[len(ms) // 2], 4), 'fastest_tenth_ms': round(ms[len(ms) // 10], 4),
            'slowest_ms': round(ms[-1], 4), 'env_steps_per_s': n * T / (ms[len(ms) // 2] / 1e3)}
    print(json.dumps(line), flush=True)
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true', help='one repetition of each case (for a kernel trace)')
    ap.add_argument('--monitor', action='store_true',
                    help='attach the on-device episode monitor: every line also carries mean_episode_return, the mean of '
                         'the last 10 polled episode returns per actor (null before an episode has finished)')
    ap.add_argument('--device-noise', action='store_true',
                    help='draw the exploration noise inside the launches from the env\'s Philox stream (attach_noise): no '
                         'eps tensor is made or read')
    ap.add_argument('--episode-lens', type=int, nargs=2, metavar=('LO', 'HI'), default=None,
                    help='the rollout cases with an episode clock per actor: actor a has episodes of LO + a %% (HI - LO + 1) '
                         'steps (the loop case is not run)')
    ap.add_argument('--task', default=None, choices=['drift', 'reach', 'arm'],
                    help='single calls on this task (see the top; arm: at obs-dim 2 x action-dim + 2)')
    ap.add_argument('--arm-shape', action='store_true', help="with --task drift: arm's obs-dim, 2 x action-dim + 2")
    ap.add_argument('--random-resets', action='store_true', help='with --task reach | arm: episodes drawn from a reset stream')
    ap.add_argument('--calls', type=int, default=60)
    ap.add_argument('--actors', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=128)
    ap.add_argument('--action-dim', type=int, default=6)
    ap.add_argument('--episode-len', type=int, default=16)
    ap.add_argument('--label', default='', help='copied into the --task line')
    ap.add_argument('--disturbance', type=float, default=0.0, metavar='S',
                    help='with --random-resets: per-step disturbances of scale S in [0, 1] drawn inside the launch '
                         '(attach_resets(disturbance=S)); 0: none')
    args = ap.parse_args()
    if args.random_resets and args.task not in ('reach', 'arm'):
        ap.error('--random-resets goes with --task reach')
    if args.disturbance and not args.random_resets:
        ap.error('--disturbance is drawn from the reset stream: give --random-resets')
    if args.task:
        lines = bench_task_calls(args)
        if args.out:
            with open(args.out, 'a') as f:
                for ln in lines:
                    f.write(json.dumps(ln) + '\n')
        return
    reps, warmup = (1, 1) if args.quick else (args.reps, args.warmup)
    lines = bench_rollouts(reps, warmup, ROLLOUTS, args.monitor, args.device_noise, args.episode_lens)
    if not args.episode_lens:
        lines += bench_loop(reps, warmup, monitor=args.monitor, device_noise=args.device_noise)
    if args.out:
        with open(args.out, 'w') as f:
            for ln in lines:
                f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
