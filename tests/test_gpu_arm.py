"""GPU tier (-m gpu): the `arm` task (surreal_amd/env/tasks.py) on the device -- the fill kernel, the per-step launch
(arm_env_step_kernel) and EnvLanes::step_arm inside ppo_window_task_kernel, lstm_window_task_kernel, the four
ddpg_rollout_kernel actors and the evaluation kernels (single-set and SETS), each <..., SMX_TASK_ARM> at 4, 8 and 16 actors
per workgroup.  Shapes (arm_cases.py): J = 1 (D = 4), 2, 30 (D = 62: the row's last lane); hidden (32, 32) and the ragged
(28, 20), an LSTM of 10 units; n = 5 (a tail block) or 20; episodes of 5 over calls of 7 + 6 steps, two episode ends
inside; n_step 3 for DDPG, windows (3, 2) for PPO (reach_cases').

  1. every recorded (obs, action, obs_next, reward) row, fed to the host arm_step, reproduces obs_next and reward;
  2. 4, 8 and 16 actors per workgroup leave the same bytes;
  3. with the reset stream each episode's first row is arm_reset_state's; two envs of 4 (actor_base 0 and 4) leave the
     bytes of one env of 8; one call of 13 steps and calls of 3 + 4 + 6 leave the bytes of 7 + 6;
  4. the monitor's fp64 returns are the step-order sums of the host rewards;
  5. evaluate and the snapshot sets equal the recording launches' monitor, as uint64, and the host definition;
  6. one launch against the float64 restatement (tests/rollout_fp64_ref.py on arm_cases.ArmEnv) at the project's 1e-5,
     at seeds under which the restatement ALONE keeps MARGIN from every clip, clamp and ReLU kink;
  7. states saturated at both limits with the goal at its extremes.

Everything but 6 is an equality of bits.  Measured on an MI355X (`pytest -s` prints the figures again): the largest error
against the restatement is 0.097 of the bound (cells, lstm_window-J30-n5; every field outside the LSTM state at most 0.022).
48 tests with test_gpu_arm_learning.py, 6.8 s together."""
import numpy as np
import pytest
import torch

import arm_cases as AC
import device_eval_cases as EV
import reach_resets_cases as RR
import rollout_envelope_cases as EC
from surreal_amd import kernels as KN
from surreal_amd.env import tasks as TK
from surreal_amd.env.synthetic_env import SyntheticEnv, SyntheticVecEnv

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BLOCKS = (4, 8, 16)
CASES = [AC.tuned(c) for c in AC.CASES]
IDS = [c.id for c in CASES]
BIT_CASES = CASES + AC.BITS_ONLY                      # (the equalities of bits: also the case no seed tunes)
BIT_IDS = [c.id for c in BIT_CASES]
PI_F = np.float32(3.1415927)
_RUNS = {}


def spare_run(c, apw):
    """the case with the reset stream attached on a ring with rows to spare, at a forced block size (once per module)"""
    if (c.id, apw) not in _RUNS:
        x = AC.setup_resets(c, DEV)
        got, rows = AC.run(x, apw)
        assert rows == x.rows and x.resets.episode == 1 + sum(AC.CALLS) // AC.EP
        _RUNS[(c.id, apw)] = (got, x, rows, AC.monitor_returns(x.venv.monitor, c.n))
    return _RUNS[(c.id, apw)]


def test_fill_kernel_gives_the_host_definition_bit_for_bit():
    K = KN.default_kernels()
    n = 5
    for J in (1, 2, 30):
        out = torch.empty(n, 2 * J + 2, device=DEV)
        for base in (0, 2 ** 32 - 5):
            for e in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3):
                K.reset_fill((AC.RSEED, base, e), out, task='arm')
                want = TK.arm_reset_state(AC.RSEED, base + np.arange(n), e, J)
                assert AC.bits(out.cpu().numpy(), want), (J, base, e)
    v = out[:, 30:60].cpu().numpy()
    assert (v == 0).all() and not np.signbit(v).any()


@pytest.mark.parametrize('J', [1, 30])
def test_step_matches_the_host_env_bit_for_bit(J):
    n, L_ = 70, 3                                        # (one thread per actor: more than one wavefront)
    D = 2 * J + 2
    venv = SyntheticVecEnv(n, D, J, episode_len=L_, device=DEV, task='arm')
    mon = venv.attach_monitor(capacity=4)
    rs = venv.attach_resets(AC.RSEED, actor_base=2 ** 32 - n)
    assert torch.equal(venv.reset(), rs.states(0)) and rs.episode == 1
    hosts = [SyntheticEnv(D, J, episode_len=L_, task='arm', resets=(AC.RSEED, 2 ** 32 - n + a)) for a in range(n)]
    for h in hosts:
        h._reset()
    returns = [[0.0] for _ in range(n)]
    acts = torch.randn(7, n, J, generator=torch.Generator().manual_seed(4)) * 1.5
    for s in range(7):
        state = venv.step(acts[s].to(DEV)).cpu()
        for a, h in enumerate(hosts):
            obs, r, done, _ = h._step(acts[s, a].numpy())
            returns[a][-1] += r
            if done:
                obs, _ = h._reset()
                returns[a].append(0.0)
            assert AC.bits(state[a].numpy(), obs['low_dim']['flat_inputs']), (s, a)
    assert rs.episode == 3
    assert AC.monitor_returns(mon, n) == [r[:2] for r in returns]
    assert mon.ep_reward.cpu().tolist() == [r[2] for r in returns]
    venv.detach_resets()
    venv.step(acts[0].to(DEV))
    venv.step(acts[1].to(DEV))                           # (the clock was at 1: this step ends the episode)
    assert torch.equal(venv.state, venv.init_state)


def test_saturated_states_and_extreme_goals():
    """theta at +-PI_F, omega at +-1, the goal at the corners of its square, actions that push outwards and back: the
    per-step launch and the one-launch windows against the host step"""
    n, J, L_ = 8, 2, 4
    D = 2 * J + 2
    sat = np.zeros((n, D), np.float32)
    for a in range(n):
        sgn = 1.0 if a % 2 == 0 else -1.0
        sat[a, :J] = sgn * PI_F
        sat[a, J:2 * J] = sgn * (1.0 if a < 4 else -1.0)
        sat[a, 2 * J:] = [-0.25 if a & 1 else np.float32(0.25) - np.float32(2.0 ** -25),
                          -0.25 if a & 2 else np.float32(0.25) - np.float32(2.0 ** -25)]
    venv = SyntheticVecEnv(n, D, J, episode_len=L_, device=DEV, task='arm')
    venv.init_state.copy_(torch.as_tensor(sat))
    venv.reset()
    s = sat.copy()
    acts = torch.tensor([5.0, -5.0, 0.3]).view(3, 1, 1).expand(3, n, J).contiguous()
    for t in range(3):
        state = venv.step(acts[t].to(DEV)).cpu().numpy()
        s, _ = TK.arm_step(s, acts[t].numpy())
        assert AC.bits(state, s), t
    assert (np.abs(s[:, :J]) <= PI_F).all() and (np.abs(s[:, J:2 * J]) <= 1.0).all()
    # the one-launch kernels from the same rows: every recorded row is the host step's
    for c in (CASES[1], CASES[3], CASES[6]):
        x = AC.setup(c._replace(n=n), DEV, wrap=False)
        x.venv.init_state.copy_(torch.as_tensor(sat))
        x.venv.reset()
        got, rows = AC.run(x, 8)
        AC.check_rows(got, x, rows)
        first = got['obs'].numpy()[:n].reshape(n, -1)[:, :D]
        assert AC.bits(first, sat)


@pytest.mark.parametrize('c', BIT_CASES, ids=BIT_IDS)
def test_rows_hold_the_host_step_and_the_reset_stream_at_every_block_size(c):
    first = None
    for apw in BLOCKS:
        got, x, rows, mon = spare_run(c, apw)
        if first is None:
            first = got
            returns = AC.check_rows(got, x, rows, resets=(AC.RSEED, 0))            # (1), (3)
            if returns is not None:
                assert mon == returns                                               # (4)
                assert all(len(r) == 2 for r in mon)
        EC.same_bits(got, first)                                                    # (2)
        assert mon == spare_run(c, BLOCKS[0])[3]


@pytest.mark.parametrize('variant', [dict(), dict(layernorm=True), dict(param_noise='normal', n=8),
                                     dict(layernorm=True, param_noise='normal', n=8)], ids=['plain', 'ln', 'pop', 'popln'])
def test_ddpg_actors_whole_steps_and_monitor_returns(variant):
    """n_step 1 records every step: the four actors of the launch on host chains over the recorded actions, (1) and (4)"""
    # (a population's block holds the actors of ONE agent: agents of 4 actors run at 4 actors per workgroup)
    for apw in ((4, 0) if 'param_noise' in variant else BLOCKS):
        got, want = AC.whole_steps(DEV, apw=apw, **variant)
        assert got == want and all(len(r) == 2 for r in got)


@pytest.mark.parametrize('c', BIT_CASES, ids=BIT_IDS)
def test_other_cuts_into_calls_leave_the_same_bytes(c):
    got = spare_run(c, 8)[0]
    for calls in ((13,), (3, 4, 6)):
        x = AC.setup_resets(c, DEV)
        one, rows = AC.run(x, 8, calls=calls)
        assert rows == x.rows
        EC.same_bits(one, got)


@pytest.mark.parametrize('cid', ['window-J1-n5', 'lstm_window-J30-n20', 'ddpg-J1-n20'])
def test_two_envs_of_four_record_what_one_of_eight_records(cid):
    c = [q for q in BIT_CASES if q.id == cid][0]
    for apw in (4, 8):
        (big, gb), small = AC.split_envs(c, DEV, apw=apw)
        RR.same_actors(gb, small, big.rows)
        assert AC.monitor_returns(big.venv.monitor, 8) == sum((AC.monitor_returns(x.venv.monitor, 4) for x, _ in small), [])


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_one_launch_meets_the_float64_restatement(c):
    """rtol = atol = 1e-5 on every float field (rollout_envelope_cases.TOL), rows written, dones and the rows never
    written exact"""
    want = None
    for apw in (4, 16, 0):
        x = AC.setup(c, DEV, wrap=False)
        if want is None:
            want, wrows, written, pol = AC.restatement(x)
            print(c.id, 'input conditions', AC.input_conditions(pol))
        got, rows = AC.run(x, apw)
        assert rows == wrows
        errs = EC.worst_errors(got, want, written)
        print('%s block %d: error / bound %s' % (c.id, apw, {k: round(v, 3) for k, v in errs.items()}))
        assert max(errs.values()) <= 1.0, (apw, errs)


# ---- (5) evaluation ------------------------------------------------------------------------------------------------------------

POLICIES = [EV.Policy('mlp-arm-J2', 'mlp', 'arm', 6, 2, (32, 32)),
            EV.Policy('mlp-arm-J30-ragged', 'mlp', 'arm', 62, 30, EV.RAGGED),
            EV.Policy('lstm-arm-J1', 'lstm', 'arm', 4, 1, (32, 32)),
            EV.Policy('lstm-arm-J30', 'lstm', 'arm', 62, 30, EV.RAGGED),
            EV.Policy('ddpg-arm-J2-ragged', 'ddpg', 'arm', 6, 2, EV.RAGGED),
            EV.Policy('ddpg-arm-J30', 'ddpg', 'arm', 62, 30, (32, 32))]
SHAPES = [(5, 3, 7), (9, 2, 4)]                            # (n, E, L): 15 rows, 18 rows


def all_blocks(venv, agent, E, resets):
    got = [EV.evaluate(venv, agent, E, resets, None, apw) for apw in BLOCKS + (0,)]
    assert got[0].dtype == np.float64 and got[0].shape == (venv.n, E)
    for g in got[1:]:
        assert EV.same_f64(g, got[0])
    return got[0]


@pytest.mark.parametrize('p', POLICIES, ids=lambda q: q.id)
def test_evaluate_and_snapshot_sets_are_the_recording_launches_bit_for_bit(p):
    for n, E, L_ in SHAPES:
        agent, cfg = EV.make_agent(p, n)
        other, _ = EV.make_agent(p, n, seed=11)
        for resets in (None, (EV.RSEED, EV.FIRST_EPISODES[1], 2 ** 32 - n)):
            venv = EV.make_env(p, n, L_, DEV)
            got = all_blocks(venv, agent, E, resets)
            want = EV.recorded_returns(p, n, E, L_, agent, cfg, DEV, resets)
            assert EV.same_f64(got, want), (n, E, L_, resets, got, want)
            assert np.isfinite(got).all() and (got != 0).any()
            if p.family != 'lstm':          # (an LSTM's state carries over episode ends in a serial run: not the same)
                assert EV.same_f64(got, EV.serial_returns(p, n, E, L_, agent, cfg, DEV, resets))
            # two snapshots in one launch: this agent's and another's
            snaps = venv.eval_snapshots(agent, 2)
            snaps.store(0)
            snaps.store(1, other)
            kw = {} if resets is None else dict(resets=resets)
            for apw in BLOCKS:
                sets = snaps.evaluate(E, actors_per_workgroup=apw, **kw).cpu().numpy()
                assert sets.shape == (2, n, E)
                assert EV.same_f64(sets[0], got) and EV.same_f64(sets[1], EV.evaluate(venv, other, E, resets))
            assert not EV.same_f64(sets[0], sets[1])


@pytest.mark.parametrize('p', [POLICIES[0], POLICIES[2], POLICIES[5]], ids=lambda q: q.id)
def test_zero_policy_returns_are_the_host_definition(p):
    for n, E, L_ in SHAPES:
        agent, _ = EV.make_agent(p, n)
        EV.constant_policy(agent, 0.0)
        for resets in (None, (EV.RSEED, EV.FIRST_EPISODES[1], 2 ** 32 - n)):
            venv = EV.make_env(p, n, L_, DEV)
            got = all_blocks(venv, agent, E, resets)
            want = AC.host_eval_returns(p.A, n, E, L_, 0.0, resets, venv.init_state.cpu().numpy())
            assert EV.same_f64(got, want), (n, E, L_, resets, got, want)
