"""What a save and a restore of a device-resident run cost (surreal_amd/utils/run_state.py).

    python scripts/bench_run_state.py [--algo ddpg|ppo|both] [--reps R] [--out FILE]

Builds scripts/train_reach.py's loop objects ((32, 32) policies, its learner settings) on the `drift` env with a monitor
and a noise stream attached, at
  ddpg: 1024 actors, D = 17, A = 6, UniformReplay memory_size 333 333 (the reference's DDPG replay);
  ppo:  1024 actors, D = 376, A = 17, FIFOReplay of 8 * actors windows of 10 steps;
runs two chunks of 16 steps (every table, carry and workspace exists, the learner has learned), then times, R times each,
  save: the state_dict() / train_state_dict() calls + run_state.save_run   (device -> pinned host, torch.save, os.replace)
  load: run_state.load_run + the load_* calls + one synchronisation         (torch.load, host -> device, in place)
and prints one JSON line per algorithm: the median and the range of both in seconds, and the file's size."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import torch  # noqa: E402

SHAPES = {'ddpg': dict(actors=1024, D=17, A=6, memory_size=333333), 'ppo': dict(actors=1024, D=376, A=17, memory_size=None)}
T = 16


def build(algo, actors, D, A, memory_size):
    import train_reach as TR
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    torch.manual_seed(0)
    folder = os.path.join(tempfile.gettempdir(), 'surreal_amd_run_state_bench')
    if algo == 'ppo':
        from surreal_amd.agent import PPOAgent as Agent
        from surreal_amd.learner import PPOLearner as Learner
        from surreal_amd.replay import FIFOReplay as Replay
        cfg = TR.ppo_configs(D, A, actors, folder)
    else:
        from surreal_amd.agent import DDPGAgent as Agent
        from surreal_amd.learner.ddpg import DDPGLearner as Learner
        from surreal_amd.replay import UniformReplay as Replay
        cfg = TR.ddpg_configs(D, A, actors, folder)
    if memory_size:
        cfg[0].replay.memory_size = memory_size
    learner, replay = Learner(*cfg), Replay(*cfg)
    agent = Agent(*cfg, agent_id=0, agent_mode='training')
    agent.attach_learner(learner)
    agent.fetch_parameter()
    venv = SyntheticVecEnv(actors, D, A, episode_len=50, seeds=list(range(actors)))
    venv.attach_monitor(capacity=8)
    venv.attach_noise(seed=1)
    B, learns = cfg[0].replay.batch_size, 0
    for _ in range(2):
        if algo == 'ppo':
            venv.ppo_rollout_into(agent, replay, T)
            while len(replay) >= B:
                learner.learn(venv.to_batch(replay.sample_batch(B, copy=False)))
                learns += 1
        else:
            venv.ddpg_rollout_into(agent, replay, T)
            stage = learner.staging_fields(B)
            for _ in range(4):
                f = replay.sample_batch(B, out=stage)
                learner.learn({'obs': {'low_dim': {'flat_inputs': f['obs']}},
                               'obs_next': {'low_dim': {'flat_inputs': f['obs_next']}}, 'actions': f['actions'],
                               'rewards': f['rewards'].view(B, 1), 'dones': f['dones'].view(B, 1)})
                learns += 1
        learner.publish_parameter(learns, message='chunk')
        agent.fetch_parameter()
    assert learns > 0
    return venv, agent, replay, learner


def measure(algo, reps):
    from surreal_amd.utils import run_state as RS
    shape = SHAPES[algo]
    venv, agent, replay, learner = build(algo, **shape)
    path = os.path.join(tempfile.mkdtemp(prefix='run_state_bench_'), 'run.pt')
    save_s, load_s = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        RS.save_run(path, env=venv.state_dict(), agent=agent.state_dict(), replay=replay.state_dict(),
                    learner=learner.train_state_dict())
        save_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        parts = RS.load_run(path)
        learner.load_train_state_dict(parts['learner'])
        replay.load_state_dict(parts['replay'])
        venv.load_state_dict(parts['env'])
        agent.load_state_dict(parts['agent'])
        torch.cuda.synchronize()
        load_s.append(time.perf_counter() - t0)
    size = os.path.getsize(path)
    os.remove(path)
    rng = lambda xs: [round(min(xs), 4), round(max(xs), 4)]  # noqa: E731
    return dict(kind='run_state', algo=algo, hidden=[32, 32], steps_before=2 * T, reps=reps, file_bytes=size,
                save_s=round(statistics.median(save_s), 4), save_s_range=rng(save_s),
                load_s=round(statistics.median(load_s), 4), load_s_range=rng(load_s),
                **{k: v for k, v in shape.items() if v is not None})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--algo', choices=['ddpg', 'ppo', 'both'], default='both')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='append the lines to this file too')
    args = ap.parse_args()
    for algo in (['ddpg', 'ppo'] if args.algo == 'both' else [args.algo]):
        line = json.dumps(measure(algo, args.reps))
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
