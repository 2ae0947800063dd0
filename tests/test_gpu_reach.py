"""GPU tier (-m gpu): the `reach` task (surreal_amd/env/tasks.py) inside the one-launch rollouts -- ppo_window_task_kernel,
lstm_window_task_kernel and ddpg_rollout_kernel<..., SMX_TASK_REACH> at 4, 8 and 16 actors per workgroup -- and in the
per-step launch (reach_env_step_kernel).  Shapes (reach_cases.py): (D, A) = (3, 1), (6, 2), (63, 21); hidden 8 and 4, 8
LSTM units; 5 actors (a partial 4-actor block) or 20; episodes of 5 steps over calls of 4, 5 and 3 steps, so two episode
ends fall inside; rings that wrap; some cases with the episode monitor and the noise stream attached.

  1. env bits: whatever the actor's GEMMs round to, the host reach_step applied to a recorded observation and action gives
     the recorded next observation and reward bit for bit (DDPG: through the n-step sum, formed as nstep_reward forms it);
  2. step() against the host env on given actions, a terminal step included, the monitor's returns with it;
  3. one launch against the float64 restatement at the project's 1e-5, under input conditions the restatement alone meets;
  4. 4, 8 and 16 actors per workgroup leave the same bytes;
  5. the monitor's returns equal those of host chains stepped with the recorded actions;
  6. task='drift' through the task entry points leaves the bytes of the entry points they forward to.

Measured on an MI355X (`pytest -s` prints the figures again): the largest error against the restatement is 0.043 of the
bound (cells, lstm_window-63-21-n20; every other field at most 0.027), episode returns 0.015 of theirs; everything else
in this file is an equality of bits.  26 tests with test_gpu_reach_learning.py, 3.5 s together.
"""
import numpy as np
import pytest
import torch

import ddpg_rollout_cases as DC
import reach_cases as RC
import rollout_envelope_cases as EC
from reach_cpu_kernels import np_nstep_sum
from surreal_amd import _lib as L
from surreal_amd.env import tasks as TK
from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv

pytestmark = pytest.mark.gpu

BLOCKS = (4, 8, 16)
CASES = [RC.tuned(c) for c in RC.CASES]
IDS = [c.id for c in CASES]
_RUNS = {}


def wrapped_run(c, apw):
    """the case on a ring that wraps, at a forced block size (run once per module)"""
    if (c.id, apw) not in _RUNS:
        x = RC.setup(c, 'cuda', wrap=True)
        got, rows = RC.run(x, apw)
        assert rows == x.rows > x.capacity
        _RUNS[(c.id, apw)] = (got, x)
    return _RUNS[(c.id, apw)]


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def window_rows(got, c):
    n, N = got['obs'].shape[0], RC.N_STEP
    return (got['obs'].numpy().reshape(n, N, c.D), got['actions'].numpy().reshape(n, N, c.A),
            got['rewards'].numpy().reshape(n, N), got['obs_next'].numpy().reshape(n, c.D))


@pytest.mark.parametrize('c', [c for c in CASES if c.family != 'ddpg'], ids=[i for i in IDS if not i.startswith('ddpg')])
def test_window_rows_hold_the_host_step_bit_for_bit_at_every_block_size(c):
    first = None
    for apw in BLOCKS:
        got, x = wrapped_run(c, apw)
        obs, act, rew, nxt = window_rows(got, c)                 # every ring row is a written window: the ring wrapped
        assert np.abs(act).max() <= 1.0 and np.isfinite(obs).all()
        for u in range(RC.N_STEP):
            sn, r = TK.reach_step(obs[:, u], act[:, u])
            assert bits(sn, obs[:, u + 1] if u + 1 < RC.N_STEP else nxt), (apw, u)
            assert bits(r, rew[:, u]), (apw, u)
        first = first or got
        EC.same_bits(got, first)
    # and the last observation of every actor is a state the task can be in: its goals are the reset state's
    goals = got['state'][:, 2 * c.A:]
    assert torch.equal(goals, x.venv.init_state.cpu()[:, 2 * c.A:])


def ddpg_chains(c, apw):
    """a DDPG case on a ring with rows to spare -> per closing step k the transition (j, tau) and the rows of all actors"""
    x = RC.setup(c, 'cuda', wrap=False)
    got, rows = RC.run(x, apw)
    assert rows == x.rows
    t, closings = 0, []
    for _ in range(sum(RC.CALLS)):
        if t >= RC.N_STEP - 1:
            closings.append((t - RC.N_STEP + 1, t))
        t = 0 if t + 1 >= RC.EP else t + 1
    return got, closings, x


@pytest.mark.parametrize('c', [c for c in CASES if c.family == 'ddpg'], ids=[i for i in IDS if i.startswith('ddpg')])
def test_ddpg_rows_hold_the_host_step_bit_for_bit(c):
    """Transition j of an episode holds (s_j, a_j), the state after step j + 2 and the 3-step reward.  Rows of one
    episode chain: reach_step(s_j, a_j) gives s_{j+1} of the next row; where the rows j, j + 1, j + 2 are all recorded
    (j = 0 in an episode of 5: the last two starts of an episode never close), obs_next and the n-step sum follow from
    recorded values alone"""
    n, N = c.n, RC.N_STEP
    got, closings, x = ddpg_chains(c, 4)
    f = {k: got[k].numpy() for k in DC.FIELDS}
    gpow = np.array([pow(RC.GAMMA, e) for e in range(N)])
    row = lambda k: slice(k * n, (k + 1) * n)  # noqa: E731
    chained = summed = 0
    for k, (j, tau) in enumerate(closings):
        sn, r = TK.reach_step(f['obs'][row(k)], f['actions'][row(k)])
        if k + 1 < len(closings) and closings[k + 1][0] == j + 1:
            assert bits(sn, f['obs'][row(k + 1)]), k
            chained += 1
        if k + N - 1 < len(closings) and closings[k + N - 1][0] == j + N - 1:
            rews, s_last = [], None
            for u in range(N):
                s_last, ru = TK.reach_step(f['obs'][row(k + u)], f['actions'][row(k + u)])
                rews.append(ru)
            assert bits(s_last, f['obs_next'][row(k)]), k
            full = np.zeros((n, tau + 1), np.float32)
            full[:, j:] = np.stack(rews, 1)
            assert bits(np_nstep_sum(full, gpow, N, tau), f['rewards'][row(k)].reshape(-1)), k
            summed += 1
        assert float(f['dones'][row(k)].min()) == float(f['dones'][row(k)].max()) == float(tau + 1 >= RC.EP)
    assert chained >= 4 and summed >= 2


@pytest.mark.parametrize('c', [c for c in CASES if c.family == 'ddpg'], ids=[i for i in IDS if i.startswith('ddpg')])
def test_ddpg_block_sizes_leave_the_same_bytes(c):
    first = None
    for apw in BLOCKS:
        got, _ = wrapped_run(c, apw)
        first = first or got
        EC.same_bits(got, first)


def test_ddpg_n_step_1_rows_are_whole_steps():
    """n_step 1: every step closes, a row is (s, a, r, s') of one step -- each the host step's, bit for bit"""
    from surreal_amd.replay import UniformReplay
    n, D, A = 5, 6, 2
    lc, ec, sc = DC.configs(D, A, n, hidden=(8, 4), n_step=1, noise_type='normal', memory_size=n * 12)
    agent = DC.make_agent(lc, ec, sc)
    venv = SyntheticVecEnv(n, D, A, episode_len=RC.EP, device='cuda', task='reach')
    replay = UniformReplay(lc, ec, sc)
    for T in RC.CALLS:
        venv.ddpg_rollout_into(agent, replay, T)
    f = EC.ring_fields(replay, DC.FIELDS)
    sn, r = TK.reach_step(f['obs'].numpy(), f['actions'].numpy())
    assert bits(sn, f['obs_next'].numpy()) and bits(r, f['rewards'].numpy().reshape(-1))
    assert float(f['dones'].sum()) == 2 * n


def test_step_matches_the_host_env_bit_for_bit():
    n, D, A, L_ = 70, 63, 21, 3                      # (one thread per actor: more than one wavefront)
    venv = SyntheticVecEnv(n, D, A, episode_len=L_, device='cuda', task='reach')
    mon = venv.attach_monitor(capacity=4)
    hosts = [SyntheticEnv(D, A, episode_len=L_, seed=a, task='reach') for a in range(n)]
    returns = [[0.0] for _ in range(n)]
    acts = torch.randn(7, n, A, generator=torch.Generator().manual_seed(4)) * 1.5
    for s in range(7):
        state = venv.step(acts[s].cuda()).cpu()
        for a, h in enumerate(hosts):
            obs, r, done, _ = h._step(acts[s, a].numpy())
            returns[a][-1] += r
            if done:
                obs, _ = h._reset()
                returns[a].append(0.0)
            assert bits(state[a].numpy(), obs['low_dim']['flat_inputs']), (s, a)
    assert mon.ep_count.tolist() == [2] * n
    assert mon.done_reward.cpu()[:, :2].tolist() == [r[:2] for r in returns]
    assert mon.ep_reward.cpu().tolist() == [r[2] for r in returns]


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_one_launch_meets_the_float64_restatement(c):
    """rtol = atol = 1e-5 on every float field, rows written, dones and the rows never written exact"""
    want = None
    for apw in (4, 16, 0):
        x = RC.setup(c, 'cuda', wrap=False)
        if want is None:
            want, wrows, written, pol = RC.restatement(x)
            print(c.id, 'input conditions', RC.input_conditions(pol))
        got, rows = RC.run(x, apw)
        assert rows == wrows
        errs = EC.worst_errors(got, want, written)
        if c.streams:
            # the monitor's finished episodes against the restatement's: an episode's sum within the bound of its terms
            per_actor = {}
            for a, reward, steps in x.venv.monitor.poll():
                per_actor.setdefault(a, []).append((reward, steps))
            worst = 0.0
            for a in range(c.n):
                assert len(per_actor[a]) == len(pol.env.finished)
                for (reward, steps), (w, mag, length) in zip(per_actor[a], pol.env.finished):
                    assert steps == length
                    worst = max(worst, abs(reward - float(w[a])) / (EC.TOL * (length + float(mag[a])) + 1e-6))
            errs['episode returns'] = worst
        print('%s block %d: error / bound %s' % (c.id, apw, {k: round(v, 3) for k, v in errs.items()}))
        assert max(errs.values()) <= 1.0, (apw, errs)


@pytest.mark.parametrize('c', [c for c in CASES if c.family != 'ddpg' and c.streams],
                         ids=[c.id for c in CASES if c.family != 'ddpg' and c.streams])
def test_monitor_returns_equal_host_chains_on_the_recorded_actions(c):
    """windows of 3 steps, 2 apart, cover every step of an episode of 5: the recorded actions drive n host envs, whose
    episode returns the monitor must hold to the bit (fp64 sums of the same fp32 rewards in step order)"""
    x = RC.setup(c, 'cuda', wrap=False)
    got, rows = RC.run(x, 8)
    _, act, rew, _ = window_rows({k: v[:rows] for k, v in got.items() if k != 'state'}, c)
    n = c.n
    mon = x.venv.monitor
    assert mon.ep_count.tolist() == [2] * n
    for e in range(2):                                  # episode e: windows 2 e (steps 0-2) and 2 e + 1 (steps 2-4)
        steps = np.concatenate([act[2 * e * n:(2 * e + 1) * n], act[(2 * e + 1) * n:(2 * e + 2) * n, 1:]], 1)
        for a in range(n):
            h = SyntheticEnv(c.D, c.A, episode_len=RC.EP, seed=a, task='reach')
            h._reset()
            total = 0.0
            for u in range(RC.EP):
                _, r, done, _ = h._step(steps[a, u])
                total += r
            assert done and float(mon.done_reward[a, e]) == total, (e, a)


def test_drift_through_the_task_entry_points_leaves_the_same_bytes(monkeypatch):
    """SMX_TASK_DRIFT forwards: a drift env run through smx_synth_*_task_f32 against the same run through the entry
    points the facade calls for 'drift'"""
    def through(redirect):
        orig = L.call

        def call(name, *args):
            if redirect and name == 'smx_synth_ppo_window_rollout_f32':
                return orig('smx_synth_ppo_window_rollout_task_f32', args[0], L.SMX_TASK_DRIFT, args[1])
            if redirect and name == 'smx_synth_ddpg_rollout_f32':
                return orig('smx_synth_ddpg_rollout_task_f32', args[0], L.SMX_TASK_DRIFT, args[2])
            if redirect and name == 'smx_synth_env_step_f32':
                return orig('smx_synth_task_env_step_f32', *args[:-1], L.SMX_TASK_DRIFT, args[-1])
            return orig(name, *args)
        out = {}
        with monkeypatch.context() as m:
            m.setattr(L, 'call', call)
            for c in (CASES[1], CASES[3], CASES[6]):
                out[c.id] = RC.run(RC.setup(c, 'cuda', task='drift'), 4)[0]
            venv = SyntheticVecEnv(9, 7, 3, episode_len=2, device='cuda')
            acts = torch.randn(3, 9, 3, generator=torch.Generator().manual_seed(0)).cuda()
            out['step'] = {'states': torch.stack([venv.step(acts[s]).clone() for s in range(3)]).cpu()}
        return out
    a, b = through(False), through(True)
    for k in a:
        EC.same_bits(a[k], b[k])
