"""What an evaluation of the deterministic policy costs on the device (GPU box), three ways on the same parameters:

  (a) per_step   the loop scripts/train_reach.py uses by default: a second env, E L iterations of act_batch /
                 forward_actor + step(), the monitor polled at the end;
  (b) rollout    ppo_rollout_into / ddpg_rollout_into with the eval_deterministic agent into a scratch replay, T = E L
                 (the env reset onto episode 0 of the held-out stream first; a monitor attached, polled at the end);
  (c) evaluate   SyntheticVecEnv.evaluate: n E rows x L steps in one launch, the returns copied to the host.

Each call is timed on the host from its first statement to the arrival of the returns (all three end in a device -> host
copy).  Configurations: `small` 64 actors x 4 episodes x 50 steps, hidden 32 / 32, J = 2; `big1` / `big4` 1024 actors x 1 / 4
episodes x 128 steps, hidden 300 / 200, A = 6; task reach, held-out episodes of a reset stream.  Rounds interleave
configurations, algorithms and variants; one JSON line per (configuration, algorithm, variant, round) with the median of
`calls` calls, then one line per (configuration, algorithm, variant) with the rounds' medians and their range.

    python scripts/bench_eval.py [--rounds 5] [--calls 60] [--configs small,big1,big4] [--algos ppo,ddpg]
                                 [--variants per_step,rollout,evaluate] [--out FILE]

--sets K[,K..]: several parameter sets on the same episodes (DeviceEvalSnapshots) -- per (configuration, algorithm, K) the
host time of `sequential`, K evaluate calls and one copy of the [K, n, E] returns, against `sets`, the one K-set launch and
one copy; the same rounds, calls and lines (`sets_rounds`), after a line that says the two leave the same bits."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import train_reach as TR  # noqa: E402
from surreal_amd.env.synthetic_env import SyntheticVecEnv  # noqa: E402

CONFIGS = {'small': dict(n=64, E=4, L=50, hidden=[32, 32], J=2),
           'big1': dict(n=1024, E=1, L=128, hidden=[300, 200], J=6),
           'big4': dict(n=1024, E=4, L=128, hidden=[300, 200], J=6)}
SEED = 3


def workloads(algo, n, E, L, hidden, J):
    """-> {variant: a function that runs one evaluation and returns the [n E] returns on the host}"""
    D, A = 3 * J, J
    TR.HIDDEN = list(hidden)
    if algo == 'ppo':
        from surreal_amd.agent import PPOAgent as Agent
        from surreal_amd.replay import FIFOReplay as Replay
        cfg = TR.ppo_configs(D, A, n, '/tmp/surreal_amd_bench_eval')
        cfg[0].replay.memory_size = n * (E * (L // cfg[0].algo.n_step) + 2)
    else:
        from surreal_amd.agent import DDPGAgent as Agent
        from surreal_amd.replay import UniformReplay as Replay
        cfg = TR.ddpg_configs(D, A, n, '/tmp/surreal_amd_bench_eval')
        cfg[0].replay.memory_size = 2 * n * E * L
    torch.manual_seed(SEED)
    agent = Agent(*cfg, agent_id=1, agent_mode='eval_deterministic_local')

    def env():
        venv = SyntheticVecEnv(n, D, A, episode_len=L, seeds=list(range(n)), task='reach')
        venv.attach_resets(SEED)
        return venv, venv.attach_monitor(capacity=max(2, E))

    def polled(mon):
        got = mon.poll()
        assert len(got) == n * E
        return np.array([r for _, r, _ in got])
    step_env, step_mon = env()

    def per_step():
        step_env.resets.episode = 0
        step_env.reset()
        for _ in range(E * L):
            if algo == 'ppo':
                actions, _ = agent.act_batch(step_env.state, eps=None)
            else:
                actions = agent.model.forward_actor(step_env.state)
            step_env.step(actions)
        return polled(step_mon)
    roll_env, roll_mon = env()
    replay = Replay(*cfg)

    def rollout():
        roll_env.resets.episode = 0
        roll_env.reset()
        if algo == 'ppo':
            roll_env.ppo_rollout_into(agent, replay, E * L)
            while len(replay):
                replay.sample_batch(min(len(replay), replay.memory_size), copy=False)
        else:
            roll_env.ddpg_rollout_into(agent, replay, E * L)
        return polled(roll_mon)
    eval_env = SyntheticVecEnv(n, D, A, episode_len=L, seeds=list(range(n)), task='reach')
    out = torch.empty(n, E, dtype=torch.float64, device=eval_env.device)

    def evaluate():
        return eval_env.evaluate(agent, E, resets=(SEED, 0), out=out).cpu().numpy().reshape(-1)
    return {'per_step': per_step, 'rollout': rollout, 'evaluate': evaluate}


def set_workloads(algo, K, n, E, L, hidden, J):
    """--sets: K parameter sets of one architecture on the same held-out episodes -> {variant: a function that runs one
    evaluation of all K and returns the [K n E] returns on the host}: `sequential`, K SyntheticVecEnv.evaluate calls into
    the rows of one tensor and one device -> host copy; `sets`, DeviceEvalSnapshots.evaluate: one launch, one copy"""
    D, A = 3 * J, J
    TR.HIDDEN = list(hidden)
    if algo == 'ppo':
        from surreal_amd.agent import PPOAgent as Agent
        cfg = TR.ppo_configs(D, A, n, '/tmp/surreal_amd_bench_eval')
    else:
        from surreal_amd.agent import DDPGAgent as Agent
        cfg = TR.ddpg_configs(D, A, n, '/tmp/surreal_amd_bench_eval')
    agents = []
    for k in range(K):
        torch.manual_seed(SEED + k)
        agents.append(Agent(*cfg, agent_id=1 + k, agent_mode='eval_deterministic_local'))
    venv = SyntheticVecEnv(n, D, A, episode_len=L, seeds=list(range(n)), task='reach')
    out = torch.empty(K, n, E, dtype=torch.float64, device=venv.device)
    snaps = venv.eval_snapshots(agents[0], K)
    for k, ag in enumerate(agents):
        snaps.store(k, ag)

    def sequential():
        for k, ag in enumerate(agents):
            venv.evaluate(ag, E, resets=(SEED, 0), out=out[k])
        return out.cpu().numpy().reshape(-1)

    def sets():
        return snaps.evaluate(E, resets=(SEED, 0), out=out).cpu().numpy().reshape(-1)
    return {'sequential': sequential, 'sets': sets}


def main_sets(args):
    """--sets K[,K..]: per (configuration, algorithm, K) the two variants of set_workloads, the protocol of the other
    mode (interleaved rounds, the median of `calls` calls a round, the rounds' range); the two must agree bit for bit"""
    ks = [int(k) for k in args.sets.split(',')]
    work = {(c, a, K): set_workloads(a, K, **CONFIGS[c])
            for c in args.configs.split(',') for a in args.algos.split(',') for K in ks}
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
    for (c, a, K), w in work.items():
        got = {v: [f() for _ in range(3)][-1] for v, f in w.items()}
        emit({'what': 'sets_agreement', 'config': c, 'algo': a, 'sets': K, **CONFIGS[c],
              'same_bits': bool(np.array_equal(got['sequential'].view(np.uint64), got['sets'].view(np.uint64)))})
    rounds = {}
    for r in range(args.rounds):
        for (c, a, K), w in work.items():
            for v, f in w.items():
                ms = [timed(f) for _ in range(args.calls)]
                rounds.setdefault((c, a, K, v), []).append(statistics.median(ms))
    for (c, a, K, v), m in rounds.items():
        emit({'what': 'sets_rounds', 'config': c, 'algo': a, 'sets': K, 'variant': v, 'calls': args.calls, **CONFIGS[c],
              'round_medians_ms': [round(x, 4) for x in m], 'min_ms': round(min(m), 4),
              'median_of_rounds_ms': round(statistics.median(m), 4), 'max_ms': round(max(m), 4)})
    if args.out:
        with open(args.out, 'w') as f:
            for ln in lines:
                f.write(json.dumps(ln) + '\n')


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=60)
    ap.add_argument('--configs', default='small,big1,big4')
    ap.add_argument('--algos', default='ppo,ddpg')
    ap.add_argument('--variants', default='per_step,rollout,evaluate')
    ap.add_argument('--out', default=None)
    ap.add_argument('--sets', default=None, help='K[,K..]: time K sequential evaluate calls against one K-set launch')
    args = ap.parse_args()
    if args.sets:
        return main_sets(args)
    variants = args.variants.split(',')
    work = {(c, a): workloads(a, **CONFIGS[c]) for c in args.configs.split(',') for a in args.algos.split(',')}
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
    for (c, a), w in work.items():
        got = {}
        for v in variants:
            for _ in range(3):
                got[v] = w[v]()              # (all three in (actor, episode) order)
        # the three agree on what they measure: (a) and (b) to the monitor's round(., 6), (c) the raw sums
        ref = got.get('evaluate')
        emit({'what': 'agreement', 'config': c, 'algo': a, **CONFIGS[c],
              'max_abs_difference_from_evaluate': {v: float(np.max(np.abs(got[v] - ref))) for v in got if ref is not None}})
    rounds = {}
    for r in range(args.rounds):
        for (c, a), w in work.items():
            for v in variants:
                ms = [timed(w[v]) for _ in range(args.calls)]
                rounds.setdefault((c, a, v), []).append(statistics.median(ms))
                emit({'what': 'eval_calls', 'config': c, 'algo': a, 'variant': v, 'round': r, 'calls': args.calls,
                      'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)})
    for (c, a, v), m in rounds.items():
        emit({'what': 'eval_rounds', 'config': c, 'algo': a, 'variant': v, **CONFIGS[c],
              'round_medians_ms': [round(x, 4) for x in m], 'min_ms': round(min(m), 4),
              'median_of_rounds_ms': round(statistics.median(m), 4), 'max_ms': round(max(m), 4)})
    if args.out:
        with open(args.out, 'w') as f:
            for ln in lines:
                f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
