"""DDPG with camera observations on one GPU, actors on the device: SyntheticVecEnv.ddpg_rollout_into with a camera agent
(per step: CNN perception of the stacked frames, the actor, one smx_synth_ddpg_pixel_step launch that steps, renders
the new frame and writes the closing transitions' uint8 pixel / pixel_next rows into the replay's ring), then
sample_batch into the learner's staging buffers and learn().  The shape of the reference's block-lifting pixel
configuration (ddpg_configs.py:176-228): camera 3 x 84 x 84, frame_stacks 3, n_step 3, conv_spec 16/32 channels,
kernels 8/4, strides 4/2, 200 features; low-dim 17, actor 300/200, critic 400/300, A 6.

  1. the rollout alone, n actors x T steps (default 256 x 128): ms per rollout, median / min / max of --reps runs,
     env-steps/s;
  2. the loop: one rollout chunk of --chunk-steps steps, then --learn-iters x (sample --batch into staging -> learn):
     env-steps/s and learner samples/s;
  3. the host path (SyntheticEnv + FrameStackWrapper + DDPGAgent.act + ExpSenderWrapperSSARNStepBootstrap, one actor
     after the other) for --host-steps steps at the same shape, for context;
  4. the new launch's bytes per step (from the shapes) -- with --stats CSV (rocprofv3 --kernel-trace --stats of a
     --trace run) also the per-step split between perception, actor and the new launch, and its bytes / kernel time.

--trace: only a warm-up and --trace-rollouts rollouts (the run to put under rocprofv3).  Prints one JSON line per
measurement."""
import argparse
import collections
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_RATE = 6.3e12                 # B/s: the achievable device-to-device copy rate of an MI355X (MI355X_MICROARCH.md)


def step_bytes(n, D, A, C, H, W, S, emit=True):
    """bytes smx_synth_ddpg_pixel_step moves in a non-final step: frame reads and writes, the low-dimensional step"""
    F = C * H * W
    writes = F + S * F + (2 * S * F if emit else 0)           # history, next observation, pixel + pixel_next
    reads = (S - 1) * F + ((2 * S - 1) * F if emit else 0)    # history frames of the stacks
    low = 4 * (2 * D + 2 * A + 2 + 3 * D + 3 * A + 3) + 8 * A + 4 * A * 2   # state, carries, ring rows, OU, mu, eps
    return n * (writes + reads + low)


def pool_step_bytes(n, D, A, C, H, W, S):
    """bytes smx_synth_ddpg_pixel_pool_step moves in a non-final step (--frame-pool): the new frame into the pool and the
    next observation, the observation's older frames out of the pool, two counters and the actor a row"""
    F = C * H * W
    low = 4 * (2 * D + 2 * A + 2 + 3 * D + 3 * A + 3) + 8 * A + 4 * A * 2
    return n * ((1 + S) * F + (S - 1) * F + 20 + low)


def kernel_split(path, T_total):
    """the --stats CSV -> per-step microseconds of perception, actor and the new launch"""
    groups = collections.OrderedDict((('pixel_step', 0.0), ('actor', 0.0), ('perception', 0.0), ('other', 0.0)))
    calls = collections.Counter()
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns, c = row['Name'], float(row['TotalDurationNs']), int(row['Calls'])
            # the actor's three layers (smx_mlp3_forward_f32) are the gemm32_kernel<true> launches; the stem's fc layer
            # writes a strided view of the perception output (gemm32_kernel<false>), and the low-dimensional columns
            # are one torch copy (elementwise_kernel)
            if 'ddpg_pixel_step_kernel' in name or 'ddpg_pixel_pool_step_kernel' in name:
                g = 'pixel_step'
            elif 'gemm32_kernel<true>' in name:
                g = 'actor'
            elif any(s in name for s in ('conv', 'im2col', 'flatten', 'gemm', 'elementwise_kernel_manual_unroll')):
                g = 'perception'
            else:
                g = 'other'
            groups[g] += ns
            calls[g] += c
    return {k: {'us_per_step': v / 1e3 / T_total, 'launches_per_step': calls[k] / T_total} for k, v in groups.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--actors', type=int, default=256)
    ap.add_argument('--steps', type=int, default=128)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--capacity', type=int, default=40000)
    ap.add_argument('--chunk-steps', type=int, default=16)
    ap.add_argument('--learn-iters', type=int, default=16)
    ap.add_argument('--loop-chunks', type=int, default=6)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--host-steps', type=int, default=3)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--trace-rollouts', type=int, default=2)
    ap.add_argument('--stats', default=None, help='rocprofv3 kernel-stats CSV of a --trace run')
    ap.add_argument('--frame-pool', action='store_true',
                    help='replay.device_frame_pool: every frame once in a pool, two counters a row')
    args = ap.parse_args()
    n, T = args.actors, args.steps
    D, A, (C, H, W), S, N = 17, 6, (3, 84, 84), 3, 3
    F = C * H * W
    shape = {'actors': n, 'steps': T, 'camera': [C, H, W], 'frame_stacks': S, 'n_step': N, 'low_dim': D,
             'actor': [300, 200], 'critic': [400, 300], 'A': A, 'conv_spec': [[16, 32], [8, 4], [4, 2], 200]}
    if args.stats:
        T_total = T * (args.trace_rollouts + 1)
        by = (pool_step_bytes if args.frame_pool else step_bytes)(n, D, A, C, H, W, S)
        split = kernel_split(args.stats, T_total)
        us = split['pixel_step']['us_per_step']
        print(json.dumps({'what': 'ddpg_pixel_kernel_split', **shape, 'rollouts_traced': args.trace_rollouts + 1,
                          'split': split, 'pixel_step_bytes': by, 'pixel_step_bytes_per_s': by / (us * 1e-6),
                          'share_of_copy_rate': by / (us * 1e-6) / COPY_RATE}), flush=True)
        return

    from surreal_amd.agent import DDPGAgent
    from surreal_amd.env.synthetic_env import SyntheticVecEnv
    from surreal_amd.learner.ddpg import DDPGLearner
    from surreal_amd.main.ddpg_configs import ddpg_learner_config, ddpg_env_config, ddpg_session_config
    from surreal_amd.replay import UniformReplay
    lc = ddpg_learner_config()
    lc.algo.n_step = N
    lc.algo.exploration.noise_type = 'ou_noise'
    lc.replay.memory_size = args.capacity
    lc.replay.batch_size = args.batch
    if args.frame_pool:
        lc.replay.device_frame_pool = True
    ec = ddpg_env_config(D, A, num_agents=n, pixel=(S * C, H, W))
    ec.frame_stacks = S
    sc = ddpg_session_config()
    agent = DDPGAgent(lc, ec, sc, agent_id=0, agent_mode='training')
    venv = SyntheticVecEnv(n, D, A, episode_len=1000, device='cuda', pixel=(C, H, W), frame_stacks=S)
    eps = torch.randn(T, n, A, device='cuda')
    replay = UniformReplay(lc, ec, sc)
    row_bytes = (20 if args.frame_pool else 2 * S * F) + 4 * (2 * D + A + 2)
    ring = {'capacity_rows': args.capacity, 'row_bytes': row_bytes, 'ring_gb': args.capacity * row_bytes / 1e9,
            'frame_pool': bool(args.frame_pool)}
    if args.frame_pool:
        from surreal_amd.replay.frame_pool import default_pool_steps
        ring['pool_gb'] = default_pool_steps(args.capacity, n, N, S) * n * F / 1e9
    venv.ddpg_rollout_into(agent, replay, T, eps=eps)                  # warm-up (tables, workspaces, code)
    torch.cuda.synchronize()
    if args.trace:
        for _ in range(args.trace_rollouts):
            venv.ddpg_rollout_into(agent, replay, T, eps=eps)
        torch.cuda.synchronize()
        print(json.dumps({'what': 'ddpg_pixel_trace_run', **shape, 'rollouts': args.trace_rollouts + 1}), flush=True)
        return

    # ---- 1. the rollout ------------------------------------------------------------------------------------------
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        venv.ddpg_rollout_into(agent, replay, T, eps=eps)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    med = float(np.median(times))
    print(json.dumps({'what': 'ddpg_pixel_rollout', **shape, **ring, 'reps': args.reps, 'ms_median': round(med, 3),
                      'ms_min': round(min(times), 3), 'ms_max': round(max(times), 3),
                      'env_steps_per_s': n * T / (med * 1e-3), 'pixel_step_bytes_per_step':
                      (pool_step_bytes if args.frame_pool else step_bytes)(n, D, A, C, H, W, S)}), flush=True)

    # ---- 2. the loop: rollout chunk -> learn iterations from the ring ----------------------------------------------
    learner = DDPGLearner(lc, ec, sc)
    B, Tc = args.batch, args.chunk_steps
    ceps = torch.randn(Tc, n, A, device='cuda')
    stage = learner.staging_fields(B)

    def learn_once():
        f = replay.sample_batch(B, out=stage)
        return learner.learn({'obs': {'pixel': {'camera0': f['pixel']}, 'low_dim': {'flat_inputs': f['obs']}},
                              'obs_next': {'pixel': {'camera0': f['pixel_next']},
                                           'low_dim': {'flat_inputs': f['obs_next']}},
                              'actions': f['actions'], 'rewards': f['rewards'].view(B, 1),
                              'dones': f['dones'].view(B, 1)})
    venv.ddpg_rollout_into(agent, replay, Tc, eps=ceps)
    for _ in range(4):
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
    print(json.dumps({'what': 'ddpg_pixel_offpolicy_loop', **shape, **ring, 'chunk_steps': Tc,
                      'learn_iters_per_chunk': args.learn_iters, 'batch': B, 'chunks': args.loop_chunks,
                      'wall_s': round(wall, 4), 'env_steps_per_s': n * Tc * args.loop_chunks / wall,
                      'learner_samples_per_s': B * args.learn_iters * args.loop_chunks / wall,
                      'critic_loss': float(st['critic_loss']), 'replay_rows': len(replay)}), flush=True)
    del learner, stage, replay
    torch.cuda.empty_cache()

    # ---- 3. the host path at the same shape, a few steps ------------------------------------------------------------
    from surreal_amd.env import ExpSenderWrapperSSARNStepBootstrap, FrameStackWrapper
    from surreal_amd.env.synthetic_env import SyntheticEnv
    from surreal_amd.session import Config
    sent = []
    envs = [ExpSenderWrapperSSARNStepBootstrap(
        FrameStackWrapper(SyntheticEnv(D, A, episode_len=1000, seed=a, pixel=(C, H, W)),
                          Config(frame_stacks=S, frame_stack_concatenate_on_env=True)), lc, sc, sink=sent.append)
        for a in range(n)]
    obs = [e.reset()[0] for e in envs]
    agent.pre_episode()
    agent.act(obs[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.host_steps):
        for a, e in enumerate(envs):
            obs[a] = e.step(agent.act(obs[a]))[0]
    wall = time.perf_counter() - t0
    print(json.dumps({'what': 'ddpg_pixel_host_path', **shape, 'steps': args.host_steps, 'wall_s': round(wall, 3),
                      'ms_per_env_step_all_actors': round(wall / args.host_steps * 1e3, 2),
                      'env_steps_per_s': n * args.host_steps / wall, 'transitions': len(sent)}), flush=True)


if __name__ == '__main__':
    main()
