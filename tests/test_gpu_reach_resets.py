"""GPU tier (-m gpu): `reach` episodes drawn on the device from per-actor Philox streams (struct smx_reset_stream;
SyntheticVecEnv.attach_resets) -- the fill kernel, the per-step launch and the nine reach instantiations of the one-launch
kernels at 4, 8 and 16 actors per workgroup.  Shapes: reach_cases' (hidden 8 / 4, LSTM 8; n = 5 and 20; J = 1, 2, 21;
episodes of 5 over calls of 4, 5 and 3 steps).

  1. the fill kernel gives tasks.reach_reset_state's bits, both counter words carrying;
  2. step(): the state after a closing step is states(e), reset() gives states(episode) and advances;
  3. the three one-launch families with a stream attached: (a) the block sizes leave the same bytes; (b) the rings hold
     what n host chains over SyntheticEnv(task='reach', resets=(seed, g)) give, bit for bit; (c) the float64 restatement
     on the drawn rows (upcast: exact) within test_gpu_reach.py's bounds, under input conditions it alone meets; (d) one
     call of 12 steps leaves the bytes of 4 + 5 + 3; (e) two envs of 4 actors record what one of 8 records; (f) poll()
     returns the host chains' episode returns; (g) a disabled stream leaves the bytes of the task entry point.

Everything but (c) is an equality of bits.  Measured on an MI355X (`pytest -s` prints the figures again): the largest
error against the restatement is 0.047 of the bound (cN, lstm_window-63-21-n20; every field outside the LSTM state at most
0.012), episode returns 0.009 of theirs.  35 tests with test_gpu_reach_resets_learning.py, 6.4 s together.
"""
import numpy as np
import pytest
import torch

import reach_cases as RC
import reach_resets_cases as RR
import rollout_envelope_cases as EC
from surreal_amd import _lib as L
from surreal_amd import kernels as KN
from surreal_amd.env import tasks as TK
from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv

pytestmark = pytest.mark.gpu

BLOCKS = (4, 8, 16)
CASES = [RR.tuned(c) for c in RR.CASES]
IDS = [c.id for c in CASES]
STREAMS = [c for c in CASES if c.streams]
_RUNS = {}


def spare_run(c, apw):
    """the case with the stream attached on a ring with rows to spare, at a forced block size (run once per module)"""
    if (c.id, apw) not in _RUNS:
        x = RR.setup(c, 'cuda', wrap=False)
        got, rows = RR.run(x, apw)
        assert rows == x.rows and x.resets.episode == RR.EPISODES
        _RUNS[(c.id, apw)] = (got, x, x.venv.monitor.poll() if c.streams else None)
    return _RUNS[(c.id, apw)]


def test_fill_kernel_gives_the_host_definition_bit_for_bit():
    K = KN.default_kernels()
    n = 5
    for J in (1, 2, 21):
        out = torch.empty(n, 3 * J, device='cuda')
        for base in (0, 2 ** 32 - 5):
            for e in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3):
                K.reset_fill((RR.RSEED, base, e), out)
                want = TK.reach_reset_state(RR.RSEED, base + np.arange(n), e, J)
                assert RR.bits(out.cpu().numpy(), want), (J, base, e)
    v = out[:, 21:42].cpu().numpy()
    assert (v == 0).all() and not np.signbit(v).any()


@pytest.mark.parametrize('L_', [3, 7])
def test_step_restarts_from_the_drawn_rows(L_):
    n, J = 70, 21                                        # (one thread per actor: more than one wavefront)
    venv = SyntheticVecEnv(n, 3 * J, J, episode_len=L_, device='cuda', task='reach')
    rs = venv.attach_resets(RR.RSEED, actor_base=2 ** 32 - n)
    assert torch.equal(venv.reset(), rs.states(0)) and rs.episode == 1
    assert RR.bits(venv.state.cpu().numpy(), TK.reach_reset_state(RR.RSEED, 2 ** 32 - n + np.arange(n), 0, J))
    hosts = [SyntheticEnv(3 * J, J, episode_len=L_, task='reach', resets=(RR.RSEED, 2 ** 32 - n + a)) for a in (0, n - 1)]
    for h in hosts:
        h._reset()
    acts = torch.randn(2 * L_ + 1, n, J, generator=torch.Generator().manual_seed(4)) * 1.5
    for s in range(acts.shape[0]):
        state = venv.step(acts[s].cuda()).cpu()
        assert rs.episode == 1 + (s + 1) // L_
        if (s + 1) % L_ == 0:
            assert torch.equal(state, rs.states(rs.episode - 1).cpu()), s
        for a, h in zip((0, n - 1), hosts):
            obs, _, done, _ = h._step(acts[s, a].numpy())
            if done:
                obs, _ = h._reset()
            assert RR.bits(state[a].numpy(), RR.flat(obs)), (s, a)
    rs.episode = 2 ** 40 + 3
    assert torch.equal(venv.reset(), rs.states(2 ** 40 + 3)) and rs.episode == 2 ** 40 + 4
    venv.detach_resets()
    assert torch.equal(venv.reset(), venv.init_state)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_rings_hold_the_host_chains_bit_for_bit_at_every_block_size(c):
    first = None
    for apw in BLOCKS:
        got, x, polled = spare_run(c, apw)
        first = first or got
        EC.same_bits(got, first)
        if c.family == 'ddpg':
            RR.ddpg_chains(got, x)
        else:
            returns = RR.window_chains(got, x)
            if c.streams:                                 # (f) the monitor's returns are the chains'
                assert RR.polled_returns(polled, c.n) == RR.rounded(returns), apw


def test_ddpg_whole_steps_and_monitor_returns():
    """(f) for DDPG, where n_step 3 records no action of an episode's last two steps: n_step 1 records every step"""
    polled, want = RR.ddpg_whole_steps('cuda')
    assert RR.polled_returns(polled, 5) == RR.rounded(want)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_one_launch_meets_the_float64_restatement_on_drawn_episodes(c):
    """rtol = atol = 1e-5 on every float field, rows written, dones and the rows never written exact"""
    want = None
    for apw in (4, 16, 0):
        x = RR.setup(c, 'cuda', wrap=False)
        if want is None:
            want, wrows, written, pol = RR.restatement(x)
            print(c.id, 'input conditions', RC.input_conditions(pol))
        got, rows = RR.run(x, apw)
        assert rows == wrows
        errs = EC.worst_errors(got, want, written)
        if c.streams:
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


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_one_call_leaves_the_bytes_of_three(c):
    got, _, _ = spare_run(c, 8)
    x = RR.setup(c, 'cuda', wrap=False)
    one, rows = RR.run(x, 8, calls=(sum(RC.CALLS),))
    assert rows == x.rows and x.resets.episode == RR.EPISODES
    EC.same_bits(one, got)


@pytest.mark.parametrize('c', STREAMS, ids=[c.id for c in STREAMS])
def test_two_envs_of_four_record_what_one_of_eight_records(c):
    for apw in (4, 8):
        (big, gb), small = RR.split_envs(c, 'cuda', apw=apw)
        RR.same_actors(gb, small, big.rows)
        want = RR.polled_returns(big.venv.monitor.poll(), 8)
        assert want == sum((RR.polled_returns(x.venv.monitor.poll(), 4) for x, _ in small), [])
        assert all(len(r) == 2 for r in want)


def test_a_disabled_stream_leaves_the_bytes_of_the_task_entry_point(monkeypatch):
    """NULL or enabled == 0 forwards: a reach env with no stream run through smx_synth_*_resets_f32 with a disabled
    stream (whose other members are nonsense) against the same run through the task entry points"""
    off = L.ResetStream()
    off.seed, off.actor_base, off.episode, off.enabled = 7, -1, -1, 0

    def through(redirect):
        orig = L.call

        def call(name, *args):
            if redirect and name in ('smx_synth_ppo_window_rollout_task_f32', 'smx_synth_ddpg_rollout_task_f32',
                                     'smx_synth_task_env_step_f32'):
                q = off if redirect == 'off' else None          # (ctypes passes the structure by reference)
                return orig(name.replace('_f32', '_resets_f32').replace('rollout_task_', 'rollout_'), *args[:-1], q,
                            args[-1])
            return orig(name, *args)
        out = {}
        with monkeypatch.context() as m:
            m.setattr(L, 'call', call)
            for c in (CASES[1], CASES[3], CASES[6]):
                out[c.id] = RC.run(RC.setup(c, 'cuda'), 4)[0]
            venv = SyntheticVecEnv(9, 6, 2, episode_len=2, device='cuda', task='reach')
            acts = torch.randn(3, 9, 2, generator=torch.Generator().manual_seed(0)).cuda()
            out['step'] = {'states': torch.stack([venv.step(acts[s]).clone() for s in range(3)]).cpu()}
        return out
    a, b, c_ = through(None), through('off'), through('null')
    for k in a:
        EC.same_bits(a[k], b[k])
        EC.same_bits(a[k], c_[k])
