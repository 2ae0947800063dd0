"""Camera-observation PPO windows (GPU box), at the reference's pixel shape (BASELINE configs[3]): 256 actors x 128-step
calls, 84 x 84 x 3 frames, frame_stacks 3, (n_step, stride) = (25, 20), CNN 256 -> LSTM 100 -> 300 -> 200 -> A, episodes of
1000 steps.  One JSON line per case:

  calls   SyntheticVecEnv.ppo_rollout_into (resumable; perception -> LSTM step -> actor -> smx_synth_ppo_pixel_window_step
          per step, windows straight into the FIFO's ring) against the path it replaces for the same T from an episode
          boundary (start_rollout + rollout + emit_windows(out=reserve_batch(...))), alternating in one process, device
          events, median / min / max over the repetitions after warm-up;
  launch  the record launch alone on a closing and on a non-closing step (device events), the bytes it must move
          computed from the shapes and the share of the HBM peak that makes;
  loop    call -> FIFO -> sample_batch(copy=False) -> PPOLearner.learn, in env-steps/s.

    python scripts/bench_ppo_pixel_window_loop.py [--reps 5] [--warmup 2] [--out FILE] [--n 256] [--T 128]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import ppo_pixel_window_cases as PP  # noqa: E402
from surreal_amd.replay import FIFOReplay  # noqa: E402

PIXEL, STACKS, N_STEP, STRIDE, L, D, A = (3, 84, 84), 3, 25, 20, 1000, 17, 6
HIDDEN, RNN, FEAT = (300, 200), 100, 256
HBM_PEAK = 8.0e12               # bytes/s, HBM3E spec (6.29e12 measured with a float4 copy)
HBM_COPY = 6.29e12


def _stats(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs)}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _agent(n, windows_per_call, batch_size=64):
    return PP.make_agent(D, A, N_STEP, STRIDE, PIXEL, STACKS, hidden=HIDDEN, rnn_hidden=RNN, feat=FEAT,
                         memory_size=max(windows_per_call, batch_size), batch_size=batch_size, final_scale=0.05)


def bench_calls(reps, warmup, n, T):
    from surreal_amd.env.exp_sender_wrapper import windows_per_episode
    W = windows_per_episode(T, N_STEP, STRIDE)
    agent, (lc, ec, sc) = _agent(n, n * (W + 1))         # (a call that resumes mid-episode may close one window more)
    new_replay, old_replay = FIFOReplay(lc, ec, sc), FIFOReplay(lc, ec, sc)
    new = PP.make_venv(n, D, A, L, PIXEL, STACKS)
    old = PP.make_venv(n, D, A, L, PIXEL, STACKS)
    eps = torch.randn(T, n, A, device='cuda')
    rows = []

    def new_path():
        rows.append(new.ppo_rollout_into(agent, new_replay, T, eps=eps))

    def old_path():
        old.reset()
        old.start_rollout(T, info_width=2 * A)
        old.rollout(agent, eps=eps)
        out = old_replay.reserve_batch(n * W, old.window_shapes(N_STEP, agent),
                                       {'pixel': torch.uint8, 'pixel_next': torch.uint8})
        assert out is not None
        old.emit_windows(N_STEP, STRIDE, out=out)
        old_replay.commit_batch(n * W)

    times = {'new': [], 'old': []}
    for r in range(warmup + reps):
        for name, fn in (('new', new_path), ('old', old_path)):
            ms = _timed(fn)
            if r >= warmup:
                times[name].append(ms)
        for rp in (new_replay, old_replay):             # (the learner's pops: views, no launch)
            while len(rp):
                rp.sample_batch(min(len(rp), rp.memory_size), copy=False)
    a, b = _stats(times['new']), _stats(times['old'])
    line = {'case': 'calls', 'n': n, 'T': T, 'pixel': list(PIXEL), 'frame_stacks': STACKS, 'n_step': N_STEP,
            'stride': STRIDE, 'episode_len': L, 'reps': reps, 'windows_per_call': sorted(set(rows)),
            'ppo_rollout_into_ms': a, 'rollout_emit_windows_ms': b, 'ratio_median': a['median'] / b['median'],
            'median_excess_ms': a['median'] - b['median'], 'parent_spread_ms': b['max'] - b['min'],
            'within_parent_spread': a['median'] - b['median'] <= b['max'] - b['min'],
            'ms_per_step': {'ppo_rollout_into': a['median'] / T, 'rollout_emit_windows': b['median'] / T}}
    print(json.dumps(line), flush=True)
    return [line]


def launch_bytes(n, closing):
    """what one record launch must move at the least: every destination frame written once, every distinct source frame
    read once, the float fields of the step and (closing) of the window"""
    F = PIXEL[0] * PIXEL[1] * PIXEL[2]
    S, N, Hl = STACKS, N_STEP, RNN
    wr = (1 + S) * F                                   # the history's new frame, the next acting observation
    rd = (S - 1) * F
    step_f = 4 * (2 * D + 3 * A + D + A + 1 + 2 * A)   # state in / out, mu | eps | log_var in, the rings' slot
    if closing:
        wr += (N + 1) * S * F
        rd = (N + S - 1) * F                           # (the window's distinct frames hold pixel_next's too)
        step_f += 2 * 4 * (N * (D + 3 * A + 2) + D + 2 * Hl)
    return n * (wr + rd + step_f)


def bench_launch(reps, warmup, n):
    """the record launch alone: tau = 24 closes window 0, tau = 25 closes nothing (device events around the launch)"""
    from surreal_amd import kernels as KN
    K = KN.default_kernels()
    C, H, W = PIXEL
    S, N, adv, Hl = STACKS, N_STEP, min(N_STEP, STRIDE), RNN
    cap, Hd = 2 * n, N_STEP + STACKS
    dev = 'cuda'
    f = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    u8 = lambda *s: torch.randint(0, 256, s, device=dev, dtype=torch.uint8)  # noqa: E731
    lines = []
    for name, tau in (('closing', N - 1), ('non_closing', N)):
        r = dict(state=f(n, D), init_state=f(n, D), t=tau, episode_len=L, n_step=N, advance=adv, log_var=f(A) - 1.0,
                 noise_scale=torch.ones(n, device=dev), eps=f(n, A), cursor=0, hist=u8(n, Hd, C, H, W), hist_pos=3,
                 obs_pixel=u8(n, S * C, H, W), h_before=f(n, Hl), c_before=f(n, Hl),
                 carry={'obs': f(n, N, D), 'actions': f(n, N, A), 'rewards': f(n, N), 'pds': f(n, N, 2 * A),
                        'cells': f(n, -(-N // adv), 2, Hl)},
                 tables={'obs': f(cap, N * D), 'obs_next': f(cap, D), 'actions': f(cap, N * A), 'rewards': f(cap, N),
                         'dones': f(cap, N), 'pds': f(cap, N * 2 * A), 'cells': f(cap, 2 * Hl),
                         'pixel': u8(cap, N * S * C * H * W), 'pixel_next': u8(cap, S * C * H * W)})
        mu = torch.tanh(f(n, A))
        state0 = r['state'].clone()
        ms = []
        for i in range(warmup + reps):
            r['state'].copy_(state0)
            r['cursor'] = (i % 2) * n                   # (alternate the destination rows)
            t = _timed(lambda: K.synth_ppo_pixel_window_step(r, mu))
            if i >= warmup:
                ms.append(t)
        s = _stats(ms)
        nbytes = launch_bytes(n, name == 'closing')
        lines.append({'case': 'launch', 'step': name, 'n': n, 'reps': reps, 'ms': s, 'bytes': nbytes,
                      'GBps_at_median': nbytes / (s['median'] * 1e-3) / 1e9,
                      'share_of_hbm_peak_8TBps': nbytes / (s['median'] * 1e-3) / HBM_PEAK,
                      'share_of_measured_copy_6.29TBps': nbytes / (s['median'] * 1e-3) / HBM_COPY})
        print(json.dumps(lines[-1]), flush=True)
    return lines


def bench_loop(reps, warmup, n, T):
    from surreal_amd.env.exp_sender_wrapper import windows_per_episode
    from surreal_amd.learner import PPOLearner
    agent, (lc, ec, sc) = _agent(n, 2 * n * windows_per_episode(T, N_STEP, STRIDE))
    learner = PPOLearner(lc, ec, sc)
    agent.attach_learner(learner)
    agent.fetch_parameter()
    replay = FIFOReplay(lc, ec, sc)
    venv = PP.make_venv(n, D, A, L, PIXEL, STACKS)
    learned = [0]
    B = lc.replay.batch_size

    def call():
        venv.ppo_rollout_into(agent, replay, T)
        while len(replay) >= B:
            learner.learn(venv.to_batch(replay.sample_batch(B, copy=False)))
            learned[0] += B
        agent.fetch_parameter()

    times = []
    for r in range(warmup + reps):
        ms = _timed(call)
        if r >= warmup:
            times.append(ms)
    s = _stats(times)
    line = {'case': 'loop', 'n': n, 'T': T, 'episode_len': L, 'batch_size': B, 'horizon': lc.algo.rnn.horizon,
            'reps': reps, 'call_ms': s,
            'env_steps_per_s': {'at_median': n * T / (s['median'] * 1e-3), 'at_min_ms': n * T / (s['min'] * 1e-3),
                                'at_max_ms': n * T / (s['max'] * 1e-3)}, 'windows_learned': learned[0]}
    print(json.dumps(line), flush=True)
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--T', type=int, default=128)
    ap.add_argument('--out', default=None)
    ap.add_argument('--cases', default='calls,launch,loop')
    args = ap.parse_args()
    lines = []
    for case in args.cases.split(','):
        if case == 'calls':
            lines += bench_calls(args.reps, args.warmup, args.n, args.T)
        elif case == 'launch':
            lines += bench_launch(max(args.reps, 20), args.warmup, args.n)
        elif case == 'loop':
            lines += bench_loop(args.reps, args.warmup, args.n, args.T)
        if args.out:                                    # (after every case: a later one may fail)
            with open(args.out, 'w') as f:
                for ln in lines:
                    f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
