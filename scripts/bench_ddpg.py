"""DDPG secondary metric: samples/sec = 512 / wall(sample + learn) at
BASELINE configs[2] (HalfCheetah shapes D=17, A=6, uniform replay, batch 512), device-resident
replay shard; and the oracle (reference ATen path) on the host CPU beside it.

    --td3                          use_double_critic + use_action_regularization
    --layernorm                    use_layernorm (with --row-schedule on: the LayerNorm chains of the row schedule; with --td3
                                   as well: two LayerNorm critics, on either schedule)
    --row-schedule on|off|unset    session_config.learner.ddpg_row_schedule (unset: the learner's own choice)
    --ab NAME[,NAME...]            timing rounds only, the named variants interleaved inside every round -- td3_layers, td3_rows,
                                   ln_layers, ln_rows, ln_td3_layers, ln_td3_rows, plain (the default learner): --rounds rounds of --calls learn() calls each, one JSON line per
                                   variant (ms per call of every round, their median, min and max) appended to --jsonl
    --tree PATH                    import surreal_amd from another checkout (the parent commit beside this one, same job)
    --label TEXT                   goes into the JSON lines
    --soft-targets                 target_update soft, tau 1e-3 (the default config's is hard every 500 iterations)
    --policy-delay D               learner_config.algo.network.policy_delay = D (D > 1 implies --soft-targets); every mean is
                                   then taken over a multiple of D iterations, so it weighs the two kinds of iteration as
                                   the learner runs them
"""
import argparse, json, sys, os, time, copy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--td3', action='store_true')
ap.add_argument('--layernorm', action='store_true')
ap.add_argument('--row-schedule', choices=['on', 'off', 'unset'], default='unset')
ap.add_argument('--ab', default='')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--calls', type=int, default=300)
ap.add_argument('--jsonl', default='')
ap.add_argument('--tree', default=ROOT)
ap.add_argument('--label', default='')
ap.add_argument('--soft-targets', action='store_true')
ap.add_argument('--policy-delay', type=int, default=1)
opt = ap.parse_args()
opt.calls = -(-opt.calls // opt.policy_delay) * opt.policy_delay
sys.path.insert(0, os.path.abspath(opt.tree)); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import numpy as np
import torch
from surreal_amd import synthetic
from surreal_amd.main.ddpg_configs import ddpg_learner_config, ddpg_env_config, ddpg_session_config
from surreal_amd.learner.ddpg import DDPGLearner

B, D, A = 512, 17, 6


def make_learner(td3, row_schedule, layernorm=False):
    lc = ddpg_learner_config(); lc.replay.batch_size = B
    lc.model.use_layernorm = bool(layernorm)
    lc.algo.network.use_double_critic = lc.algo.network.use_action_regularization = bool(td3)
    if opt.soft_targets or opt.policy_delay > 1:
        lc.algo.network.target_update = {'type': 'soft', 'tau': 1e-3}
    if opt.policy_delay != 1:
        lc.algo.network.policy_delay = opt.policy_delay
    sc = ddpg_session_config()
    if row_schedule != 'unset':
        sc.learner['ddpg_row_schedule'] = row_schedule == 'on'
    return lc, DDPGLearner(lc, ddpg_env_config(D, A), sc)


if opt.ab:
    variants = {'td3_layers': (True, 'off'), 'td3_rows': (True, 'on'), 'plain': (False, 'unset'),
                'ln_layers': (False, 'off', True), 'ln_rows': (False, 'on', True),
                'ln_td3_layers': (True, 'off', True), 'ln_td3_rows': (True, 'on', True)}
    names = [n for n in opt.ab.split(',') if n]
    learners = {n: make_learner(*variants[n])[1] for n in names}
    batches = {n: [learners[n].preprocess(synthetic.make_ddpg_batch(B, D, A, seed=s)) for s in range(8)] for n in names}
    for n in names:
        for i in range(20): learners[n].learn(batches[n][i % 8])
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    for r in range(opt.rounds):
        for n in names:
            L, bs = learners[n], batches[n]
            for i in range(10): L.learn(bs[i % 8])
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(opt.calls): L.learn(bs[i % 8])
            torch.cuda.synchronize(); ms[n].append((time.perf_counter() - t0) / opt.calls * 1e3)
    for n in names:
        L = learners[n]
        rec = {'variant': n, 'label': opt.label, 'batch': B, 'D': D, 'A': A, 'calls_per_round': opt.calls, 'rounds': opt.rounds,
               'policy_delay': opt.policy_delay, 'target_update': L.target_update_type,
               'schedule': L._schedule(B, D), 'graph': L._ws.graph is not None, 'ms_per_learn_rounds': [round(v, 5) for v in ms[n]],
               'ms_per_learn_median': round(float(np.median(ms[n])), 5), 'ms_min': round(min(ms[n]), 5), 'ms_max': round(max(ms[n]), 5)}
        line = json.dumps(rec)
        print(line)
        if opt.jsonl:
            with open(opt.jsonl, 'a') as f:
                f.write(line + '\n')
    sys.exit(0)

lc, L = make_learner(opt.td3, opt.row_schedule, opt.layernorm)
print('schedule: %s (td3 %s, layernorm %s, ddpg_row_schedule %s)' % (L._schedule(B, D), opt.td3, opt.layernorm, opt.row_schedule))
batches = [L.preprocess(synthetic.make_ddpg_batch(B, D, A, seed=s)) for s in range(8)]
for i in range(20): L.learn(batches[i % 8])
torch.cuda.synchronize(); t0 = time.perf_counter(); n = -(-300 // opt.policy_delay) * opt.policy_delay
for i in range(n): st = L.learn(batches[i % 8])
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
print('DDPG learn (batch resident): %.3f ms/iter  %.3g samples/s  critic_loss %.4f' % (dt * 1e3, B / dt, st['critic_loss']))
# how much of that is the HOST: the same loop's enqueue time alone (the clock stops before the device is waited for), and the
# device's own time per iteration from events around the loop
torch.cuda.synchronize(); e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0 = time.perf_counter(); e0.record()
for i in range(n): st = L.learn(batches[i % 8])
e1.record(); th = (time.perf_counter() - t0) / n
torch.cuda.synchronize()
print('   host enqueue time per learn(): %.3f ms; device time per iteration (events): %.3f ms' % (th * 1e3, e0.elapsed_time(e1) / n))
# ---- with the uniform replay in the loop: 1e6 SSAR rows resident in HBM, sample 512 + learn ----
from surreal_amd.replay import UniformReplay
lc.replay.memory_size = 1000000
R = UniformReplay(lc, ddpg_env_config(D, A), ddpg_session_config())
g = torch.Generator(device='cuda').manual_seed(0)
for _ in range(10):
    n = 100000
    R.insert_batch({'obs': torch.randn(n, D, device='cuda', generator=g), 'obs_next': torch.randn(n, D, device='cuda', generator=g),
                    'actions': torch.rand(n, A, device='cuda', generator=g) * 2 - 1, 'rewards': torch.randn(n, device='cuda', generator=g),
                    'dones': (torch.rand(n, device='cuda', generator=g) < 0.01).float()})


def sample_and_learn():
    f = R.sample_batch(B)
    return L.learn({'obs': {'low_dim': {'flat_inputs': f['obs']}}, 'obs_next': {'low_dim': {'flat_inputs': f['obs_next']}},
                    'actions': f['actions'], 'rewards': f['rewards'].view(B, 1), 'dones': f['dones'].view(B, 1)})


for i in range(20): sample_and_learn()
torch.cuda.synchronize(); t0 = time.perf_counter(); n = 300
for i in range(n): st = sample_and_learn()
torch.cuda.synchronize(); ds = (time.perf_counter() - t0) / n
print('DDPG sample(512 of 1e6) + learn: %.3f ms/iter  %.3g samples/s  (hipGraph %s)' % (ds * 1e3, B / ds, L._ws.graph is not None))
try:
    import ddpg_oracle
    params = ddpg_oracle.make_ddpg_params(D, A, (300, 200), (400, 300), seed=3, layernorm=opt.layernorm)
    td3 = dict(use_double_critic=True, use_action_regularization=True, batch_size=B,
               params2=ddpg_oracle.make_ddpg_params(D, A, (300, 200), (400, 300), seed=4, layernorm=opt.layernorm)) if opt.td3 else {}
    O = ddpg_oracle.OracleDDPGLearner(params, A, **td3) if hasattr(ddpg_oracle, 'OracleDDPGLearner') else None
    if O is not None:
        hb = [synthetic.make_ddpg_batch(B, D, A, seed=s) for s in range(8)]
        for i in range(5): O.learn(copy.deepcopy(hb[i % 8]))
        t0 = time.perf_counter(); n = 100
        for i in range(n): O.learn(copy.deepcopy(hb[i % 8]))
        dc = (time.perf_counter() - t0) / n
        print('oracle (reference ATen path, %d threads): %.3f ms/iter  %.3g samples/s  -> x%.1f' % (torch.get_num_threads(), dc * 1e3, B / dc, dc / dt))
except Exception as e:
    print('oracle timing skipped:', repr(e))
