"""DDPG's off-policy loop on one GPU with the actors on the device: SyntheticVecEnv.ddpg_rollout_into (act, explore,
step and record n-step transitions straight into the uniform replay's ring), then sample_batch into the learner's
staging buffers and learn().

  1. the rollout alone, n actors x T steps, D -> H1 -> H2 -> A (default 1024 x 128, 17 -> 300 -> 200 -> 6), into a ring
     of 1e6 rows: the persistent kernel (one launch) and the per-step path (one actor forward + one step launch per
     step): ms per rollout, env-steps/s, and the share of the FP32 matrix peak the actor's FLOPs
     2 n T (D H1 + H1 H2 + H2 A) take;
  2. the loop: one rollout chunk, then `--learn-iters` learn iterations at batch 512 sampled with
     sample_batch(512, out=learner.staging_fields(512)): env-steps/s and learner samples/s over the whole loop.

With --calls N: only N single `ddpg_rollout_into` calls, each as a user makes it and timed by itself -> one line with
their median (and, with --param-noise, the time of DeviceParamNoise.refresh()).  --param-noise attaches per-agent
parameter-space noise (attach_param_noise, --actors-per-agent K actors an agent): the population launch; it needs --calls,
since the per-step path and the plain kernel's forced blocks have no such launch.  --layernorm: a LayerNorm actor
(use_layernorm, random gains and biases), combinable with --param-noise and --device-noise; with --calls, --per-step times
its per-step path (reference=True) instead of the one launch.

Prints one JSON line per measurement (and a summary line)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from surreal_amd.agent import DDPGAgent  # noqa: E402
from surreal_amd.env.synthetic_env import SyntheticVecEnv  # noqa: E402
from surreal_amd.learner.ddpg import DDPGLearner  # noqa: E402
from surreal_amd.main.ddpg_configs import ddpg_learner_config, ddpg_env_config, ddpg_session_config  # noqa: E402
from surreal_amd.replay import UniformReplay  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12        # MI355X, FLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--actors', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=128)
    ap.add_argument('--obs-dim', type=int, default=17)
    ap.add_argument('--hidden', type=int, nargs=2, default=[300, 200])
    ap.add_argument('--action-dim', type=int, default=6)
    ap.add_argument('--capacity', type=int, default=1000000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--noise', default='ou_noise', choices=['normal', 'ou_noise'])
    ap.add_argument('--loop-chunks', type=int, default=8)
    ap.add_argument('--chunk-steps', type=int, default=16)
    ap.add_argument('--learn-iters', type=int, default=16)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--episode-len', type=int, default=1000)
    ap.add_argument('--episode-lens', type=int, nargs=2, metavar=('LO', 'HI'), default=None,
                    help='with --calls: an episode clock per actor, actor a with episodes of LO + a %% (HI - LO + 1) steps')
    ap.add_argument('--monitor', action='store_true',
                    help='attach the on-device episode monitor: every line also carries mean_episode_return, the mean of '
                         'the last 10 polled episode returns per actor (null before an episode has finished)')
    ap.add_argument('--device-noise', action='store_true',
                    help='draw the exploration noise inside the launches from the env\'s Philox stream (attach_noise): no '
                         'eps tensor is made or read')
    ap.add_argument('--param-noise', action='store_true',
                    help='attach per-agent parameter-space noise (adaptive_normal): every agent acts from its own perturbed '
                         'copy of the actor, made and measured on the device; needs --calls')
    ap.add_argument('--actors-per-agent', type=int, default=4, help='actors that share one perturbation (a multiple of 4)')
    ap.add_argument('--layernorm', action='store_true', help='a LayerNorm behind each hidden ReLU of the actor and critic')
    ap.add_argument('--per-step', action='store_true', help='with --layernorm --calls: the per-step path (reference=True)')
    ap.add_argument('--calls', type=int, default=0, help='time this many single rollout calls, print their median and stop')
    ap.add_argument('--label', default='', help='copied into the --calls line')
    ap.add_argument('--task', default=None, choices=['drift', 'reach', 'arm'],
                    help="with --calls: the environment's dynamics at obs-dim 3 x action-dim (reach's shape; --obs-dim is "
                         'ignored; arm: at its own 2 x action-dim + 2) on the one-launch route: the plain actor, or with '
                         '--layernorm / --param-noise their instantiations on the task')
    ap.add_argument('--arm-shape', action='store_true', help="with --task drift: arm's obs-dim, 2 x action-dim + 2")
    ap.add_argument('--random-resets', action='store_true',
                    help='with --task reach | arm: draw every episode inside the launch from a reset stream (attach_resets)')
    ap.add_argument('--disturbance', type=float, default=0.0, metavar='S',
                    help='with --random-resets: per-step disturbances of scale S in [0, 1] drawn inside the launch '
                         '(attach_resets(disturbance=S)); 0: none')
    args = ap.parse_args()
    if args.param_noise and not args.calls:
        ap.error('--param-noise measures single calls: give --calls N')
    if args.per_step and not (args.layernorm and args.calls and not args.param_noise):
        ap.error('--per-step goes with --layernorm --calls N, without --param-noise')
    if args.episode_lens and not args.calls:
        ap.error('--episode-lens measures single calls of the one-launch path: give --calls N')
    if args.task and not args.calls:
        ap.error('--task measures single calls of the one-launch path: give --calls N')
    if args.random_resets and args.task not in ('reach', 'arm'):
        ap.error('--random-resets goes with --task reach')
    if args.disturbance and not args.random_resets:
        ap.error('--disturbance is drawn from the reset stream: give --random-resets')
    if args.task:
        args.obs_dim = 2 * args.action_dim + 2 if args.task == 'arm' or args.arm_shape else 3 * args.action_dim
    n, T, D, A = args.actors, args.steps, args.obs_dim, args.action_dim
    H1, H2 = args.hidden
    lc = ddpg_learner_config()
    lc.model.actor_fc_hidden_sizes = [H1, H2]
    lc.model.use_layernorm = args.layernorm
    lc.algo.exploration.noise_type = args.noise
    if args.param_noise:
        lc.algo.exploration.param_noise_type = 'adaptive_normal'
    lc.replay.memory_size = args.capacity
    lc.replay.batch_size = args.batch
    ec, sc = ddpg_env_config(D, A, num_agents=n), ddpg_session_config()
    agent = DDPGAgent(lc, ec, sc, agent_id=0, agent_mode='training')
    if args.layernorm:                         # (the defaults 1 / 0 would time an affine step of ones and zeros)
        for k, v in agent.model.actor_ln.items():
            v.copy_(torch.rand_like(v) + 0.5 if k.endswith('.W') else 0.1 * torch.randn_like(v))
    flops = 2.0 * n * T * (D * H1 + H1 * H2 + H2 * A)
    episode_len = args.episode_len
    if args.episode_lens:
        lo, hi = args.episode_lens
        episode_len = [lo + a % (hi - lo + 1) for a in range(n)]
    task = {'task': args.task} if args.task in ('reach', 'arm') else {}  # ('drift': no keyword, as before there were tasks)
    venv = SyntheticVecEnv(n, D, A, episode_len=episode_len, device='cuda', **task)
    if args.random_resets:
        venv.attach_resets(seed=3, disturbance=args.disturbance)
        venv.reset()
    mon = venv.attach_monitor() if args.monitor else None

    def returns(line):
        if mon is not None:
            mon.poll()
            line.update(mean_episode_return=mon.mean_reward(last=10), episodes=mon.num_episodes, monitor=True)
        return line
    if args.device_noise:
        venv.attach_noise(seed=1)
    eps = None if args.device_noise else torch.randn(T, n, A, device='cuda')
    if args.calls:
        return single_calls(args, agent, venv, UniformReplay(lc, ec, sc), eps)
    results = {}
    for path in ('persistent', 'per_step'):
        replay = UniformReplay(lc, ec, sc)
        if path == 'per_step':              # the per-step path: what a LayerNorm actor or an unsupported shape takes
            venv.K.synth_ddpg_rollout_supported = lambda net, ln=False: False
        try:
            venv.reset()
            venv.ddpg_rollout_into(agent, replay, T, eps=eps)           # warm-up (tables, packed copy, code)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.reps):
                venv.ddpg_rollout_into(agent, replay, T, eps=eps)
            e1.record()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / args.reps
            dev = e0.elapsed_time(e1) / 1e3 / args.reps
        finally:
            if path == 'per_step':
                del venv.K.synth_ddpg_rollout_supported
        r = {'what': 'ddpg_rollout', 'path': path, 'actors': n, 'steps': T, 'shape': [D, H1, H2, A],
             'ms_per_rollout': round(dev * 1e3, 4), 'wall_ms_per_rollout': round(wall * 1e3, 4),
             'env_steps_per_s': n * T / dev, 'actor_tflops': flops / dev / 1e12,
             'share_of_fp32_matrix_peak': flops / dev / FP32_MATRIX_PEAK, 'replay_rows': len(replay)}
        results[path] = returns(r)
        print(json.dumps(r), flush=True)

    # ---- the off-policy loop: rollout chunk -> learn iterations from the ring ------------------------------------------
    learner = DDPGLearner(lc, ec, sc)
    replay = UniformReplay(lc, ec, sc)
    venv.reset()
    B, Tc = args.batch, args.chunk_steps
    ceps = None if args.device_noise else torch.randn(Tc, n, A, device='cuda')
    venv.ddpg_rollout_into(agent, replay, Tc, eps=ceps)
    stage = learner.staging_fields(B)

    def learn_once():
        f = replay.sample_batch(B, out=stage)
        return learner.learn({'obs': {'low_dim': {'flat_inputs': f['obs']}},
                              'obs_next': {'low_dim': {'flat_inputs': f['obs_next']}}, 'actions': f['actions'],
                              'rewards': f['rewards'].view(B, 1), 'dones': f['dones'].view(B, 1)})
    for _ in range(8):
        st = learn_once()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.loop_chunks):
        venv.ddpg_rollout_into(agent, replay, Tc, eps=ceps)
        for _ in range(args.learn_iters):
            st = learn_once()
    st = dict(st)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    loop = {'what': 'ddpg_offpolicy_loop', 'actors': n, 'chunk_steps': Tc, 'learn_iters_per_chunk': args.learn_iters,
            'batch': B, 'chunks': args.loop_chunks, 'wall_s': round(wall, 4),
            'env_steps_per_s': n * Tc * args.loop_chunks / wall,
            'learner_samples_per_s': B * args.learn_iters * args.loop_chunks / wall,
            'critic_loss': float(st['critic_loss']), 'replay_rows': len(replay)}
    print(json.dumps(returns(loop)), flush=True)
    # the persistent kernel at each forced block size (the automatic pick above: 4 actors per workgroup up to one
    # workgroup per CU)
    for apw in (4, 8, 16):
        replay = UniformReplay(lc, ec, sc)
        venv.reset()
        venv.ddpg_rollout_into(agent, replay, T, eps=eps, actors_per_workgroup=apw)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            venv.ddpg_rollout_into(agent, replay, T, eps=eps, actors_per_workgroup=apw)
        e1.record()
        torch.cuda.synchronize()
        dev = e0.elapsed_time(e1) / 1e3 / args.reps
        print(json.dumps({'what': 'ddpg_rollout', 'path': 'persistent', 'actors_per_workgroup': apw, 'actors': n,
                          'steps': T, 'ms_per_rollout': round(dev * 1e3, 4), 'env_steps_per_s': n * T / dev,
                          'share_of_fp32_matrix_peak': flops / dev / FP32_MATRIX_PEAK}), flush=True)
    speedup = results['per_step']['ms_per_rollout'] / results['persistent']['ms_per_rollout']
    print(json.dumps({'what': 'summary', 'persistent_ms': results['persistent']['ms_per_rollout'],
                      'per_step_ms': results['per_step']['ms_per_rollout'], 'persistent_speedup': speedup}), flush=True)


def timed(f, k):
    """k calls of f, each between its own pair of events -> their times in ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]
    torch.cuda.synchronize()
    for e0, e1 in ev:
        e0.record()
        f()
        e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) for e0, e1 in ev)


def single_calls(args, agent, venv, replay, eps):
    n, T = args.actors, args.steps
    pn = venv.attach_param_noise(agent, seed=2, actors_per_agent=args.actors_per_agent) if args.param_noise else None
    call = lambda: venv.ddpg_rollout_into(agent, replay, T, eps=eps, reference=args.per_step)  # noqa: E731
    for _ in range(3):
        call()
    ms = timed(call, args.calls)
    line = {'what': 'ddpg_rollout_calls', 'label': args.label, 'actors': n, 'steps': T, 'calls': args.calls,
            'task': args.task, 'random_resets': args.random_resets, 'disturbance': args.disturbance, 'shape': [args.obs_dim] + args.hidden + [args.action_dim],
            'episode_len': args.episode_len,
            'layernorm': args.layernorm, 'per_step': args.per_step, 'param_noise': bool(pn), 'actors_per_agent': args.actors_per_agent if pn else None,
            'agents': pn.agents if pn else None, 'median_ms': round(ms[len(ms) // 2], 4),
            'fastest_tenth_ms': round(ms[len(ms) // 10], 4), 'slowest_ms': round(ms[-1], 4),
            'env_steps_per_s': n * T / (ms[len(ms) // 2] / 1e3)}
    if pn is not None:
        pn.refresh()
        rs = timed(pn.refresh, 20)
        line.update(refresh_median_ms=round(rs[len(rs) // 2], 4), refresh_slowest_ms=round(rs[-1], 4),
                    population_mb=round(pn.pop.numel() * 4 / 1e6, 2))
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
